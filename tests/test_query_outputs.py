"""GPU: `saf_query_scan` called through ctypes with `out` AND `out_last` -- no caller in the package asks for both, so no other
test does -- on every route of the dispatch (one wave per row, the matrix scan with one and two label tiles, 64-label and
32-label blocks with their finishing pass) and every epilogue, against the oracle's double-precision statement on the features as
stored (the 16-bit values upcast).

Per case: the status is 0; `out` is within the tolerance the project's scans are held to; `out_last` equals column L - 1 of
`out` from the SAME call bit for bit (every route stores the column from a register and `out_last` from the same register: the
one-wave-per-row kernel and the matrix scan's epilogue store `val`, the finishing pass of a block scan stores `v` to both, a raw
block scan's last launch is a matrix scan over the block that ends in column L - 1); and a call with `out = NULL` gives the same
`out_last` within the tolerance (beyond 64 labels that call runs the one-wave-per-row kernel by design: there is no [N, L] matrix
for the blocks' scores to meet in)."""

import numpy as np
import pytest
import torch

from spatially_aware_ai_amd import _abi

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-6  # (tests/test_gpu_parity.py: test_query_scan_over_more_than_64_labels, test_query_golden)
EPILOGUES = ((_abi.SAF_Q_SCORES, 3.0), (_abi.SAF_Q_SOFTMAX, 100.0), (_abi.SAF_Q_SURGERY, 1.0))
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16

# (route, D, L, dtype, padded): `padded` reads the features through feat_stride = D + 8, a view into a wider tensor whose rows
# keep their 16-byte alignment
CASES = (
    [("wave-per-row", 100, nl, F32, False) for nl in (5, 70)] + [("wave-per-row", 100, 70, F32, True)]
    + [("matrix", 512, nl, dt, False) for nl in (5, 32, 33, 64) for dt in (F32, F16, BF16)]
    + [("matrix", 512, 33, dt, True) for dt in (F32, BF16)]
    + [("blocks-64", 512, nl, dt, False) for nl in (65, 100, 129) for dt in (F32, F16)] + [("blocks-64", 512, 100, F16, True)]
    + [("blocks-32", 768, nl, F32, False) for nl in (40, 100)] + [("blocks-32", 768, 40, F32, True)]
)


def _inputs(n, d, nl, dt, padded):
    g = torch.Generator().manual_seed(1000 * d + nl)
    feats = torch.randn((n, d), generator=g)
    feats[7] = 0.0  # an all-zero row: nan_to_num gives zeros (row 0 stays: the surgery weights come from it)
    text = torch.nn.functional.normalize(torch.randn((nl, d), generator=g), dim=-1)
    stored = feats.to(dt)
    if padded:
        wide = torch.full((n, d + 8), float("nan"), dtype=dt)
        wide[:, :d] = stored
        fd = wide.cuda()[:, :d]
    else:
        fd = stored.cuda()
    return fd, stored.float(), text


def _scan(fd, text_d, epi, scale, want_out, want_last):
    from spatially_aware_ai_amd._lib import lib

    L = lib()
    n, d = fd.shape
    nl = text_d.shape[0]
    ft = {F32: _abi.SAF_F32, BF16: _abi.SAF_BF16, F16: _abi.SAF_F16}[fd.dtype]
    # poisoned: a value the scan does not store shows
    out = torch.full((n, nl), float("nan"), device=fd.device) if want_out else None
    last = torch.full((n,), float("nan"), device=fd.device) if want_last else None
    wsb = L.saf_query_workspace_bytes(nl, epi)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=fd.device)
    rc = L.saf_query_scan(fd.data_ptr(), ft, n, fd.stride(0), d, text_d.data_ptr(), nl, text_d.stride(0), epi, float(scale),
                          _abi.SAF_NORM_L2, _abi.ptr(out), _abi.ptr(last), ws.data_ptr(), wsb,
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out, last


@pytest.mark.parametrize("n", [3001, 31])
@pytest.mark.parametrize("route,d,nl,dt,padded", CASES,
                         ids=[f"{r}-D{d}-L{nl}-{str(dt).split('.')[-1]}{'-padded' if p else ''}" for r, d, nl, dt, p in CASES])
def test_out_and_out_last_together(oracle, route, d, nl, dt, padded, n):
    from spatially_aware_ai_amd._lib import lib

    fd, fo, text = _inputs(n, d, nl, dt, padded)
    assert fd.stride(0) == (d + 8 if padded else d) and fd.data_ptr() % 16 == 0
    text_d = text.cuda()
    for epi, scale in EPILOGUES:
        what = f"{route}: epilogue {epi}, D {d}, {nl} labels, {n} rows, {dt}"
        want = oracle.query_scan(fo, text, epi, scale=scale, normalize=True).numpy()
        rc, out, last = _scan(fd, text_d, epi, scale, True, True)
        assert rc == 0, f"{what}: rc {rc}: {lib().saf_last_error().decode()}"
        out, last = out.cpu().numpy(), last.cpu().numpy()
        err = np.abs(out.astype(np.float64) - want)
        print(f"{what}: out max abs err {np.nanmax(err):.3g}, out_last != column: {int((last != out[:, nl - 1]).sum())}")
        np.testing.assert_allclose(out, want, rtol=RTOL, atol=ATOL, err_msg=what)
        assert np.array_equal(last, out[:, nl - 1]), f"{what}: out_last is not the last column of the same call"
        rc, none, only = _scan(fd, text_d, epi, scale, False, True)
        assert rc == 0 and none is None, f"{what}: out = NULL: rc {rc}: {lib().saf_last_error().decode()}"
        np.testing.assert_allclose(only.cpu().numpy(), last, rtol=RTOL, atol=ATOL, err_msg=what + " (out = NULL)")
