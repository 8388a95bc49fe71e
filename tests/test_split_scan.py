"""The split scan (saf_query.hip, query_split_kernel): fp32 text-query scores out of fp16 matrix instructions.

Every fp32 operand is cut into two fp16 pieces under a power-of-two scale (the rows' scale follows their running maximum), the dot
products are hi.hi + hi.lo + lo.hi with fp32 accumulation.  What the cut drops is bounded by 3 x 2^-22 of sum_k |a_k b_k| per
score; these tests hold it to 4 x 2^-22 of that sum (+ the fp32 accumulation's own rounding) against a float64 scan -- on ordinary
CLIP-like rows and on rows built to break a fixed scale: magnitudes from 1e-30 to 1e30, late spikes, leading zeros, denormals.
Reference semantics: clipfusion.py:899-934, clip_seem_fusion.py:507-511 (the oracle's query_scan restates them)."""
import os

import numpy as np
import pytest
import torch

from spatially_aware_ai_amd import _abi

pytestmark = pytest.mark.gpu

CUT = 4.0 * 2.0 ** -22   # the pieces' rounding + the dropped lo.lo term, relative to sum |a b|
ACC = 3.0e-7              # fp32 accumulation over <= 512 terms on ordinary rows (what the exact-fp32 chain shows against float64)
ACC_WORST = 96 * 2.0 ** -24  # its worst case: one term dominates and each of a row's 96 matrix instructions rounds the running
                             # sum once (the fp32 chain this replaces rounds it 512 times: 512 x 2^-24)


def _scan(feats, text, epi=_abi.SAF_Q_SCORES, scale=1.0, normalize=False):
    from spatially_aware_ai_amd.clipfusion import _query_scan
    return _query_scan(feats, text, epi, scale=scale, normalize=normalize)


def _raw_bound(f64, t64):
    """per (row, label): sum_k |a_k b_k| in float64"""
    return np.abs(f64) @ np.abs(t64).T


def _check_raw(feats, text, what, acc=ACC):
    """raw scores (no normalisation): the split scan against float64, error relative to sum |a b|"""
    got = _scan(feats.cuda(), text.cuda()).double().cpu().numpy()
    f64, t64 = feats.float().double().numpy(), text.double().numpy()
    want = f64 @ t64.T
    mag = _raw_bound(f64, t64)
    bound = mag * (CUT + acc)
    err = np.abs(got - want)
    bad = (err > bound + 1e-44) & (mag < 1e37)   # (beyond: the score itself may leave fp32's range)
    if bad.any():
        r, c = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} scores off by more than the cut allows; first at row {r}, "
                             f"label {c}: got {got[r, c]!r}, float64 {want[r, c]!r}, sum |a b| {mag[r, c]!r}")
    ok = (mag < 1e37) & (mag > 1e-30)
    return float((err[ok] / mag[ok]).max())


@pytest.mark.parametrize("nl", [5, 33, 63, 64])
def test_split_scan_is_fp32_faithful(nl):
    n, d = 6007, 512
    g = torch.Generator().manual_seed(100 + nl)
    feats = torch.nn.functional.normalize(torch.randn((n, d), generator=g), dim=-1) * (0.2 + torch.rand((n, 1), generator=g))
    text = torch.nn.functional.normalize(torch.randn((nl, d), generator=g), dim=-1)
    worst = _check_raw(feats, text, f"{nl} labels")
    # and not worse than twice the fp32 matrix instructions' own distance from float64 + the cut
    os.environ["SAF_Q_SPLIT"] = "0"
    try:
        exact = _scan(feats.cuda(), text.cuda()).double().cpu().numpy()
    finally:
        del os.environ["SAF_Q_SPLIT"]
    f64, t64 = feats.double().numpy(), text.double().numpy()
    exact_err = float((np.abs(exact - f64 @ t64.T) / _raw_bound(f64, t64)).max())
    assert worst <= 2.0 * exact_err + CUT, (worst, exact_err)


@pytest.mark.parametrize("fdt", [torch.float32, torch.float16, torch.bfloat16])
def test_split_scan_epilogues_against_oracle(oracle, fdt):
    """softmax / surgery / scores with the fused normalisation, the three volume dtypes, against the oracle at BASELINE's tolerance"""
    n, d = 4003, 512
    g = torch.Generator().manual_seed(5)
    feats = torch.randn((n, d), generator=g)
    feats[11] = 0.0
    fd = feats.to(fdt).cuda()
    fo = fd.float().cpu()
    for nl in (5, 63):
        text = torch.nn.functional.normalize(torch.randn((nl, d), generator=g), dim=-1)
        for epi, scale, norm in ((_abi.SAF_Q_SURGERY, 1.0, True), (_abi.SAF_Q_SOFTMAX, 100.0, True), (_abi.SAF_Q_SCORES, 3.0, True),
                                 (_abi.SAF_Q_SCORES, 1.0, False)):
            want = oracle.query_scan(fo, text, epi, scale=scale, normalize=norm)
            got = _scan(fd, text.cuda(), epi, scale=scale, normalize=norm)
            np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=1e-4, atol=2e-6, err_msg=f"epilogue {epi}, {nl} labels, {fdt}")


def test_split_scan_rows_of_any_magnitude():
    """rows and labels that a fixed fp16 scale would overflow or flush: the row scale follows the running maximum"""
    d, nl = 512, 63
    g = torch.Generator().manual_seed(9)
    base = torch.randn((64 * 14, d), generator=g)
    rows = base.clone().view(14, 64, d)
    rows[0] *= 1e30
    rows[1] *= 1e-30
    rows[2] *= 1e-40                                   # denormal features
    rows[3, :, 64:] *= 1e5                             # everything behind the first group far larger: one re-scale
    rows[4] *= torch.logspace(-6, 9, d)[None]          # a steady climb over 15 decades: re-scale after re-scale
    rows[5, :, :64] = 0.0                              # the scale cannot come from the first group
    rows[6] = 0.0
    rows[6, :, -1] = 3.0                               # one feature, the last
    rows[7] *= torch.logspace(9, -6, d)[None]          # a steady fall: late features far below the scale
    rows[8, :, 100] = 6.0e4                            # a spike above fp16's largest finite value x the scale
    rows[9] *= (10.0 ** torch.randint(-20, 20, (64, 1), generator=g).float())  # every row of a tile at another magnitude
    rows[10, :, ::2] = 0.0
    rows[11] = rows[11].abs() * 1e-3 + 1.0             # no cancellation, tiny variation around a constant
    rows[12, :, 448:] *= 1e12                          # the last group only
    rows[13] *= 65504.0
    feats = rows.view(-1, d)
    text = torch.randn((nl, d), generator=g)
    text[0] *= 1e20
    text[1] *= 1e-20
    text[2] = 0.0
    text[3, 5:] = 0.0
    text[4] *= 1e-40
    finite = _check_raw(feats, text, "magnitudes", acc=ACC_WORST)
    assert np.isfinite(finite)
    # normalised scores of the same rows: cosine values, so the bound is relative to |a| |b|-sized sums again
    keep = torch.ones(14, dtype=torch.bool)
    keep[[0, 1, 2, 9]] = False                         # (their sums of squares leave fp32's range, in the reference too)
    f = rows[keep].view(-1, d)
    t = torch.nn.functional.normalize(torch.randn((nl, d), generator=g), dim=-1)
    got = _scan(f.cuda(), t.cuda(), normalize=True).double().cpu().numpy()
    f64 = f.double().numpy()
    norm = np.sqrt((f64 * f64).sum(-1, keepdims=True))
    want = (f64 / norm) @ t.double().numpy().T
    bound = (np.abs(f64) / norm) @ np.abs(t.double().numpy()).T * (CUT + ACC_WORST)
    assert (np.abs(got - want) <= bound).all(), float((np.abs(got - want) / bound).max())


@pytest.mark.parametrize("d", [16, 48, 80, 192, 336, 528, 1024])
def test_split_scan_other_widths(d):
    """feat_dim a multiple of 16 but not of 64: the pairs behind the last full group; no full group at all; an odd number of
    64-feature groups (192: three, the conditional ring with a group in flight; 336: five and a trailing pair)"""
    n, nl = 1000, 37
    g = torch.Generator().manual_seed(d)
    feats = torch.randn((n, d), generator=g)
    feats[:, d // 2:] *= 300.0
    text = torch.randn((nl, d), generator=g)
    _check_raw(feats, text, f"D = {d}")


@pytest.mark.parametrize("d", [8, 72, 200, 520])
def test_exact_fp32_scan_other_widths(d):
    """feat_dim a multiple of 8 but not of 16: the split scan does not take it, the exact-fp32 matrix scan (query_mfma_kernel) does
    by default -- no 64-feature group at all, one / three / eight groups and a chunk of 8 behind them; both label tiles"""
    n, nl = 1000, 37
    g = torch.Generator().manual_seed(d)
    feats = torch.randn((n, d), generator=g)
    feats[:, d // 2:] *= 300.0
    text = torch.randn((nl, d), generator=g)
    _check_raw(feats, text, f"exact fp32, D = {d}")


def test_split_scan_strided_rows_and_non_finite():
    """a row stride wider than feat_dim (a view of a wider volume), and non-finite features: the row's scores are non-finite, its
    neighbours' are untouched"""
    n, d, nl = 777, 512, 20
    g = torch.Generator().manual_seed(3)
    wide = torch.randn((n, d + 64), generator=g).cuda()
    text = torch.randn((nl, d), generator=g)
    view = wide[:, :d]
    assert not view.is_contiguous()
    got = _scan(view, text.cuda()).double().cpu().numpy()
    f64, t64 = view.double().cpu().numpy(), text.double().numpy()
    assert (np.abs(got - f64 @ t64.T) <= _raw_bound(f64, t64) * (CUT + ACC)).all()
    bad = view.clone().contiguous()
    bad[5, 17] = float("inf")
    bad[40, 300] = float("nan")
    got_b = _scan(bad, text.cuda()).cpu().numpy()
    assert not np.isfinite(got_b[5]).any() and not np.isfinite(got_b[40]).any()
    ok = np.ones(n, dtype=bool)
    ok[[5, 40]] = False
    np.testing.assert_array_equal(got_b[ok], got.astype(np.float32)[ok])


@pytest.mark.parametrize("n", [1, 31, 33, 64, 257])
def test_split_scan_few_rows_and_one_label(oracle, n):
    """fewer rows than a tile, a tile and a row, whole tiles only (the staged 16-byte stores) -- with 1, 2 and 64 labels"""
    d = 512
    g = torch.Generator().manual_seed(n)
    feats = torch.randn((n, d), generator=g)
    for nl in (1, 2, 64):
        text = torch.nn.functional.normalize(torch.randn((nl, d), generator=g), dim=-1)
        _check_raw(feats, text, f"{n} rows, {nl} labels")
        for epi, scale in ((_abi.SAF_Q_SURGERY, 1.0), (_abi.SAF_Q_SOFTMAX, 100.0)):
            want = oracle.query_scan(feats, text, epi, scale=scale, normalize=True)
            got = _scan(feats.cuda(), text.cuda(), epi, scale=scale, normalize=True)
            np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=1e-4, atol=2e-6, err_msg=f"epilogue {epi}, {n} rows, {nl} labels")
            last = _query_last(feats.cuda(), text.cuda(), epi, scale)
            np.testing.assert_allclose(last.cpu().numpy(), want.numpy()[:, -1], rtol=1e-4, atol=2e-6)


def _query_last(feats, text, epi, scale):
    from spatially_aware_ai_amd.clipfusion import _query_scan
    return _query_scan(feats, text, epi, scale=scale, normalize=True, last_only=True)


@pytest.mark.parametrize("d,nl", [(768, 63), (1024, 40), (1024, 100)])
def test_split_scan_wide_features_in_blocks_of_32(oracle, d, nl):
    """feat_dim 768 / 1024 (OpenCLIP's larger towers): two 32-label tiles do not fit the LDS, so more than 32 labels run 32 at a time on
    the matrix cores with a finishing pass (rounds 1-5: the one-wave-per-row kernel)"""
    n = 2051
    g = torch.Generator().manual_seed(d + nl)
    feats = torch.randn((n, d), generator=g)
    feats[3] = 0.0
    text = torch.nn.functional.normalize(torch.randn((nl, d), generator=g), dim=-1)
    _check_raw(feats, text, f"D = {d}, {nl} labels")
    for epi, scale in ((_abi.SAF_Q_SURGERY, 1.0), (_abi.SAF_Q_SOFTMAX, 100.0), (_abi.SAF_Q_SCORES, 3.0)):
        want = oracle.query_scan(feats, text, epi, scale=scale, normalize=True)
        got = _scan(feats.cuda(), text.cuda(), epi, scale=scale, normalize=True)
        np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=1e-4, atol=2e-6, err_msg=f"epilogue {epi}, D = {d}, {nl} labels")


@pytest.mark.parametrize("fdt", [torch.bfloat16, torch.float16])
def test_split_scan_16bit_volumes_of_any_magnitude(fdt):
    """The 16-bit-volume form (query_split16_kernel): one fp16 piece per feature.  bf16 rows span fp32's range and go under the
    running scale; fp16 rows go as they are, denormals and 65504 included.  Against float64 of the SAME 16-bit values."""
    d, nl = 512, 63
    g = torch.Generator().manual_seed(21)
    rows = torch.randn((10, 64, d), generator=g)
    if fdt == torch.bfloat16:
        rows[0] *= 1e30
        rows[1] *= 1e-30
        rows[2, :, 128:] *= 1e5                            # a step behind the first group of 128
        rows[3] *= torch.logspace(-6, 9, d)[None]
        rows[4, :, :128] = 0.0
        rows[5] *= torch.logspace(9, -6, d)[None]
        rows[6] *= (10.0 ** torch.randint(-20, 20, (64, 1), generator=g).float())
        rows[7] = 0.0
        rows[7, :, -1] = -2.5
        rows[8] *= 1e-38                                   # bf16 denormals
    else:
        rows[0] *= 1.0e4                                   # up to ~5e4
        rows[0].clamp_(-65504, 65504)
        rows[1] *= 1e-6                                    # fp16 denormals
        rows[2, :, 128:] *= 1e3
        rows[3] *= torch.logspace(-7, 3, d)[None]
        rows[4, :, :128] = 0.0
        rows[7] = 0.0
        rows[7, :, -1] = 65504.0
    feats = rows.view(-1, d).to(fdt)
    text = torch.randn((nl, d), generator=g)
    text[0] *= 1e6
    text[1] *= 1e-6
    text[2] = 0.0
    _check_raw(feats, text, f"{fdt} magnitudes", acc=ACC_WORST)
    # the same through a view whose rows are not on 16-byte boundaries (row stride 520 - 4 elements): the fp32-widening form takes it
    wide = torch.zeros((feats.shape[0], d + 4), dtype=fdt)
    wide[:, :d] = feats
    got = _scan(wide.cuda()[:, :d], text.cuda()).double().cpu().numpy()
    f64, t64 = feats.float().double().numpy(), text.double().numpy()
    mag = _raw_bound(f64, t64)
    ok = mag < 1e37
    assert (np.abs(got - f64 @ t64.T)[ok] <= (mag * (CUT + ACC_WORST))[ok] + 1e-44).all()


@pytest.mark.parametrize("fdt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("d", [16, 144, 272, 384, 400, 1024])
def test_split_scan_16bit_other_widths(fdt, d):
    """16-bit volumes whose rows are not a whole number of 128-feature groups (no group at all; one group and a k-step; two groups --
    the ring with unconditional loads -- and a k-step behind them; three groups -- the conditional ring with a group in flight --
    alone and with a k-step behind them) and 1024 channels"""
    n, nl = 777, 29
    g = torch.Generator().manual_seed(d)
    feats = (torch.randn((n, d), generator=g) * 3.0).to(fdt)
    text = torch.randn((nl, d), generator=g)
    _check_raw(feats, text, f"D = {d}, {fdt}")
