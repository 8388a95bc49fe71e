"""The 7 x 7 depthwise convolution of the ConvNeXt block (csrc/saf_dwconv.hip; backbone op of BASELINE config 3's panoptic
encoder, handy_utils.py:29-161), per element:

* fp32 against the float64 statement (tests/frame_pass_reference.py): |got - exact| <= 50 * 2^-24 * S, S the sum of the absolute
  terms of that element -- derived from the kernel's 49 fmaf into an accumulator that starts at the bias, not measured;
* bf16 / fp16 bit for bit against the fp32 instantiation on the widened input, rounded once to nearest even: the two run the same
  fmaf sequence and differ only in the final store;
* the block around it: which path ran, with gamma = 1 so that the depthwise output reaches the block's output."""
import math

import pytest
import torch
import torch.nn.functional as F

import frame_pass_reference as R

pytestmark = pytest.mark.gpu

# (n, c, h, w): the smallest shape; one column; one row; today's small shape; w == kTX; w == kTX + 1 (a strip with one live pixel);
# C8 = 25 does not divide 256 (workgroups straddle strips) with a batch stride; today's two larger shapes
SHAPES = [(1, 8, 1, 1), (1, 8, 7, 1), (1, 8, 1, 9), (2, 8, 5, 3), (1, 24, 4, 4), (1, 24, 3, 5), (3, 200, 9, 6), (1, 192, 37, 41),
          (1, 384, 60, 80)]
SLICE = "slice"  # x[1:] of the (3, 200, 9, 6) tensor: a storage offset that is not 0
LOUD = "loud"    # (1, 192, 37, 41) with one channel scaled by 1e4 beside ordinary ones


def _cl(x):
    return x.cuda().contiguous(memory_format=torch.channels_last)


def _operands(case, seed_extra=0):
    n, c, h, w = (3, 200, 9, 6) if case == SLICE else (1, 192, 37, 41) if case == LOUD else case
    g = torch.Generator().manual_seed(c * 1000 + h * 10 + w + seed_extra)
    x = torch.randn(n, c, h, w, generator=g)
    if case == LOUD:
        x[:, 5] *= 1e4
    wt = torch.randn(c, 1, 7, 7, generator=g) / 7.0
    b = torch.randn(c, generator=g)
    return x, wt, b


def _tie_operands(case, dt):
    """Small-integer activations, half-integer weights and integer biases of a magnitude at which the 16-bit ulp is 1 or 2:
    every fp32 partial sum is exact, and about half of the results are exact rounding ties of `dt`."""
    n, c, h, w = (3, 200, 9, 6) if case == SLICE else case
    g = torch.Generator().manual_seed(c * 1000 + h * 10 + w + 7)
    x = torch.randint(-4, 5, (n, c, h, w), generator=g).float()
    wt = torch.randint(-4, 5, (c, 1, 7, 7), generator=g).float() * 0.5
    lo, hi = (160, 700) if dt == torch.bfloat16 else (2600, 7000)
    b = torch.randint(lo, hi, (c,), generator=g).float() * (torch.randint(0, 2, (c,), generator=g).float() * 2 - 1)
    return x, wt, b


@pytest.mark.parametrize("dt,tol", [(torch.float32, 2e-6), (torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -10)])
@pytest.mark.parametrize("n,c,h,w", [(1, 192, 37, 41), (2, 8, 5, 3), (1, 384, 60, 80)])
def test_dwconv7x7_matches_conv2d(dt, tol, n, c, h, w):
    """The first-day check, kept: the largest error over the whole tensor against the library's convolution in fp32 on the same
    (rounded) operands.  It is blind to a quiet channel beside a loud one and to the rounding of the store: the tests below."""
    from spatially_aware_ai_amd.backbones import dwconv7x7

    g = torch.Generator().manual_seed(c + h)
    x = torch.randn(n, c, h, w, generator=g).to(dt).cuda().contiguous(memory_format=torch.channels_last)
    wt = (torch.randn(c, 1, 7, 7, generator=g) / 7.0).cuda()
    b = torch.randn(c, generator=g).cuda()
    want = F.conv2d(x.float(), wt, b, padding=3, groups=c)
    got = dwconv7x7(x, wt, b)
    assert got.dtype == dt and got.is_contiguous(memory_format=torch.channels_last)
    err = (got.float() - want).abs().max() / want.abs().max()
    assert float(err) <= tol, float(err)
    got2 = dwconv7x7(x, wt, None)
    torch.testing.assert_close(got2.float(), F.conv2d(x.float(), wt, None, padding=3, groups=c), rtol=0, atol=float(tol * want.abs().max()))


@pytest.mark.parametrize("case", SHAPES + [SLICE, LOUD], ids=str)
def test_dwconv7x7_fp32_per_element(case):
    """|got - exact| <= 50 * 2^-24 * S for every element.  Largest observed err / bound on the MI355X, with / without bias:
      (1, 8, 1, 1) 0.015 / 0.013     (1, 8, 7, 1) 0.042 / 0.027      (1, 8, 1, 9) 0.063 / 0.021     (2, 8, 5, 3) 0.065 / 0.038
      (1, 24, 4, 4) 0.043 / 0.041    (1, 24, 3, 5) 0.065 / 0.038     (3, 200, 9, 6) 0.101 / 0.072   (1, 192, 37, 41) 0.123 / 0.092
      (1, 384, 60, 80) 0.138 / 0.101 slice 0.101 / 0.072             loud 0.123 / 0.092
    (the roundings of 49 terms mostly cancel: the worst element of 1.8 M is at a seventh of the bound)."""
    from spatially_aware_ai_amd.backbones import dwconv7x7

    x, wt, b = _operands(case)
    xd = _cl(x)
    if case == SLICE:
        xd, x = xd[1:], x[1:]
        assert xd.storage_offset() != 0 and xd.is_contiguous(memory_format=torch.channels_last)
    for bias in (b, None):
        got = dwconv7x7(xd, wt.cuda(), None if bias is None else bias.cuda())
        assert got.dtype == torch.float32 and got.shape == x.shape and got.is_contiguous(memory_format=torch.channels_last)
        exact, mag = R.dwconv7x7_f64(x, wt, bias)
        ratio = ((got.cpu().double() - exact).abs() / (R.DWCONV_BOUND * mag).clamp_min(1e-300)).max()
        print(f"dwconv fp32 {case} bias={bias is not None}: max err / bound = {float(ratio):.4f}")
        assert float(ratio) <= 1.0, float(ratio)
        if case == LOUD:  # the bound is per element: it holds on the ordinary channels beside the loud one
            quiet = [i for i in range(x.shape[1]) if i != 5]
            assert float(mag[:, quiet].max()) < 0.1 * float(mag[:, 5].min())


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("case", SHAPES + [SLICE], ids=str)
def test_dwconv7x7_16bit_is_the_fp32_result_rounded_once(case, dt):
    """dwconv7x7(x16) == dwconv7x7(x16.float()).to(dt), bit for bit, on N(0,1) operands and on operands that put the fp32
    results ON rounding ties.  Asserted on the tie operands: at least 1 % of the fp32 results (and at least one) lie a quarter
    ulp16 before a tie or beyond it (a truncating store would move them), and as many are exact ties (round-half-up would move
    half of those); the fp32 results are exact there, so the output also equals the float64 statement rounded once.
    Observed shares over the cases: 0.38 - 0.78 at or beyond the quarter ulp, 0.12 - 0.38 exact ties (asserted: >= 0.01 each)."""
    from spatially_aware_ai_amd.backbones import dwconv7x7

    for kind in ("normal", "ties"):
        x, wt, b = _operands(case, 1) if kind == "normal" else _tie_operands(case, dt)
        x16 = _cl(x.to(dt))
        if case == SLICE:
            x16, x = x16[1:], x[1:]
            assert x16.storage_offset() != 0
        for bias in (b, None) if kind == "normal" else (b,):
            bd = None if bias is None else bias.cuda()
            got = dwconv7x7(x16, wt.cuda(), bd)
            y32 = dwconv7x7(x16.float(), wt.cuda(), bd)
            assert got.dtype == dt and y32.dtype == torch.float32 and got.is_contiguous(memory_format=torch.channels_last)
            assert torch.equal(got, y32.to(dt)), (kind, "the 16-bit store is not the fp32 result rounded to nearest even")
        if kind == "ties":
            frac = R.ulp16_fraction(y32, dt)
            need = max(1, math.ceil(0.01 * frac.numel()))
            near, ties = int((frac >= 0.25).sum()), int((frac == 0.5).sum())
            print(f"dwconv {dt} {case}: {near / frac.numel():.3f} at or beyond a quarter ulp before the tie, {ties / frac.numel():.3f} exact ties")
            assert near >= need and ties >= need, (near, ties, frac.numel())
            exact, _ = R.dwconv7x7_f64(x.to(dt), wt, b)
            assert torch.equal(y32.cpu().double(), exact), "small integers: every fp32 partial sum is exact"
            assert torch.equal(got.cpu(), exact.float().to(dt))


# ---------------------------------------------------------------------------------------------------------------- the block
class _Counted:
    """backbones.dwconv7x7 with its calls counted and its last output kept."""

    def __init__(self, monkeypatch):
        from spatially_aware_ai_amd import backbones

        self.calls, self.out, self._real = 0, None, backbones.dwconv7x7
        monkeypatch.setattr(backbones, "dwconv7x7", self)

    def __call__(self, *a, **k):
        self.calls += 1
        self.out = self._real(*a, **k)
        return self.out


def _block(c, seed=0):
    from spatially_aware_ai_amd.backbones import _ConvNeXtBlock

    torch.manual_seed(seed)
    blk = _ConvNeXtBlock(c).cuda().eval()
    with torch.no_grad():
        blk.gamma.fill_(1.0)  # (initialised to 1e-6: the depthwise output would not reach the block's output)
    return blk


def _rest(blk, x, dw_out):
    """The block after its depthwise convolution, with the library's own operators."""
    return x + (blk.fc2(F.gelu(blk.fc1(blk.ln(dw_out.permute(0, 2, 3, 1))))) * blk.gamma).permute(0, 3, 1, 2)


def _dw_ratio(out, x, blk):
    """err / bound of a depthwise output against the float64 statement: the fp32 bound, plus half a 16-bit ulp of the rounded
    value where the output is 16 bits wide (the one rounding of the store)."""
    exact, mag = R.dwconv7x7_f64(x, blk.dw.weight, blk.dw.bias)
    bound = R.DWCONV_BOUND * mag
    if out.dtype != torch.float32:
        bound = bound + (2.0 ** -8 if out.dtype == torch.bfloat16 else 2.0 ** -11) * (exact.abs() + bound)
    return float(((out.detach().cpu().double() - exact).abs() / bound).max())


def test_convnext_block_takes_the_hip_depthwise_path(monkeypatch):
    """The block calls the HIP depthwise convolution exactly once for a channels-last input under no_grad (fp32, and bf16 under
    autocast, where the input is converted); what that call returned is within the per-element bound of the float64 statement,
    and the block's output is the rest of the block applied to it, exactly (the carry-through of the bound over LayerNorm, GELU
    and two library GEMMs is not derivable: the depthwise output is compared inside the block and the rest bit for bit)."""
    counted = _Counted(monkeypatch)
    blk = _block(192)
    x = torch.randn(1, 192, 33, 29, device="cuda").contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        got = blk(x)
        assert counted.calls == 1 and counted.out.dtype == torch.float32
        assert _dw_ratio(counted.out, x, blk) <= 1.0
        assert torch.equal(got, _rest(blk, x, counted.out))
        # gamma = 1: the depthwise output matters -- the block's output moves by far more than rounding when it is zeroed
        assert float((got - _rest(blk, x, torch.zeros_like(counted.out))).abs().max()) > 1e-2
        with torch.autocast("cuda", dtype=torch.bfloat16):
            got16 = blk(x)
            assert counted.calls == 2 and counted.out.dtype == torch.bfloat16
            assert _dw_ratio(counted.out, x.bfloat16(), blk) <= 1.0
            assert torch.equal(got16, _rest(blk, x, counted.out))


@pytest.mark.parametrize("why", ["nchw", "c12", "grad"])
def test_convnext_block_falls_back_to_the_library_convolution(monkeypatch, why):
    """An NCHW-contiguous input, a channel count that is no multiple of 8 and a pass that autograd records do not take the HIP
    path, and the block's output is the library-convolution block's."""
    counted = _Counted(monkeypatch)
    c = 12 if why == "c12" else 24
    blk = _block(c, seed=1)
    x = torch.randn(2, c, 9, 11, device="cuda")
    if why != "nchw":
        x = x.contiguous(memory_format=torch.channels_last)
    if why == "grad":
        x.requires_grad_(True)
        got = blk(x)
        assert got.requires_grad
    else:
        with torch.no_grad():
            got = blk(x)
    assert counted.calls == 0
    with torch.no_grad():
        dw = blk.dw(x.detach())
        exact, mag = R.dwconv7x7_f64(x, blk.dw.weight, blk.dw.bias)
        # the library's convolution is not ours to bound by operation count: 49 terms in any order and any fusion stay within
        # 2 * 49 roundings of the absolute sum
        assert bool(((dw.cpu().double() - exact).abs() <= 2 * 49 * 2.0 ** -24 * mag).all())
        assert torch.equal(got.detach(), _rest(blk, x.detach(), dw))
    if why == "grad":
        got.sum().backward()
        assert x.grad is not None and blk.dw.weight.grad is not None


def test_weight_cache_follows_the_weights(monkeypatch):
    """The re-laid [7, 7, C] weights are cached by address and version: an in-place update and load_state_dict are seen by the
    next call, and a call without a change reuses the cached tensors."""
    counted = _Counted(monkeypatch)
    blk = _block(24, seed=2)
    x = torch.randn(1, 24, 6, 7, device="cuda").contiguous(memory_format=torch.channels_last)
    cache = blk.__dict__["_dw_cache"]
    with torch.no_grad():
        blk(x)
        first_w = cache["w"]
        blk(x)
        assert cache["w"] is first_w and counted.calls == 2
        before = counted.out.clone()
        blk.dw.weight.mul_(2)
        blk(x)
        assert cache["w"] is not first_w and _dw_ratio(counted.out, x, blk) <= 1.0 and not torch.equal(counted.out, before)
        blk.dw.bias.add_(1.5)
        blk(x)
        assert _dw_ratio(counted.out, x, blk) <= 1.0
        other = _block(24, seed=3)
        blk.load_state_dict(other.state_dict())
        blk(x)
        assert torch.equal(blk.dw.weight, other.dw.weight) and _dw_ratio(counted.out, x, blk) <= 1.0
        assert counted.calls == 5


def test_c_entry_refusals():
    from spatially_aware_ai_amd import _abi
    from spatially_aware_ai_amd._lib import current_stream_ptr, lib

    dev = torch.device("cuda", 0)
    x, y = torch.zeros(2 * 3 * 4 * 16 + 4, device=dev), torch.full((2 * 3 * 4 * 16 + 4,), 7.0, device=dev)
    w = torch.zeros(49 * 16, device=dev)
    call = lambda xp, c, dt: lib().saf_dwconv7x7_nhwc(xp, w.data_ptr(), None, y.data_ptr(), 2, 3, 4, c, dt, current_stream_ptr())
    assert call(x.data_ptr(), 12, _abi.SAF_F32) == _abi.SAF_E_UNSUPPORTED   # channels % 8 != 0
    assert call(x.data_ptr() + 4, 16, _abi.SAF_F32) == _abi.SAF_E_INVALID   # x off a 16-byte boundary
    assert call(x.data_ptr(), 16, 7) == _abi.SAF_E_INVALID                  # no such dtype
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()), "a refused call wrote nothing"
    assert call(x.data_ptr(), 16, _abi.SAF_F32) == _abi.SAF_OK
    torch.cuda.synchronize()
    assert bool((y[:-4] == 0.0).all()) and bool((y[-4:] == 7.0).all())
