"""GPU: the wide scan (saf_query_scan_wide, saf_query_scan_wide_ex; csrc/saf_query_wide.hip) where its route depends on the caller's
layout or data: feature / text strides above feat_dim (the row-block prefetch's base), a caller's `out` at any stride and base
(vector and scalar stores, the columns beyond the result), rows with inf / NaN in them and rows at the ends of the dtype's range,
and the two reductions without L2 normalisation.

Both entry points are called through ctypes on the tensors as they lie (`_wide`), as tests/test_query_outputs.py calls the narrow
scan.  Truth is oracle.wide_scan / oracle.query_scan -- double precision on the same rounded operands -- at the bars of
tests/test_gpu_parity.py (TOL below); on top of that every layout case equals BIT FOR BIT the same scan of contiguous copies into an
output the wrapper allocates (query_scan_wide): a layout changes where bytes are read and stored, not the arithmetic.  Every case that
reaches saf_query_scan_wide_ex runs in both forms (SAF_WIDE_MFMA = 16: query_wide3_kernel, 32: query_wide2_kernel)."""
import functools

import numpy as np
import pytest
import torch

from spatially_aware_ai_amd import _abi

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
TOL = {F32: 3e-5, F16: 1e-3, BF16: 8e-3}  # tests/test_gpu_parity.py: test_wide_scan_v2_scores_and_epilogues
VAL = 3e-5                                 # fp32 reduction values; a winner's oracle score against the oracle's best
_DT = {F32: _abi.SAF_F32, F16: _abi.SAF_F16, BF16: _abi.SAF_BF16}
_NORM = {False: _abi.SAF_NORM_NONE, True: _abi.SAF_NORM_L2, "clamp": _abi.SAF_NORM_L2_CLAMP}
_ONORM = {False: 0, True: 1, "clamp": 2}
_EPI = {"scores": _abi.SAF_QW_SCORES, "vs_background": _abi.SAF_QW_VS_BACKGROUND, "row_argmax": _abi.SAF_QW_ROW_ARGMAX,
        "query_max": _abi.SAF_QW_QUERY_MAX}
_BITS = {2: torch.int16, 4: torch.int32, 8: torch.int64}
FORMS = ["16", "32"]
N_BG = 4


def _name(dt):
    return str(dt).split(".")[-1]


def _bits(t):
    return t.contiguous().view(_BITS[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _wide(feats, text, epi="scores", scale=1.0, normalize=True, n_bg=0, rescale=False, out=None, out_dtype=None, row_offset=0,
          first=False):
    """saf_query_scan_wide_ex (feat_dim 128, or `first`: saf_query_scan_wide) on `feats`, `text` and `out` exactly as they lie in
    memory"""
    from spatially_aware_ai_amd._lib import lib

    L = lib()
    assert feats.is_cuda and text.is_cuda and text.dtype == F32 and feats.stride(1) == 1 and text.stride(1) == 1
    n, d = feats.shape
    q, e, dev = text.shape[0], _EPI[epi], feats.device
    stream = torch.cuda.current_stream().cuda_stream
    idx = val = row = None
    if e in (_abi.SAF_QW_SCORES, _abi.SAF_QW_VS_BACKGROUND):
        if out is None:
            out = torch.full((n, q - n_bg), float("nan"), dtype=out_dtype or feats.dtype, device=dev)
        assert out.shape == (n, q - n_bg) and out.stride(1) == 1
    if d == 128 or first:
        assert e == _abi.SAF_QW_SCORES
        wsb = L.saf_query_wide_workspace_bytes(q, d)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        rc = L.saf_query_scan_wide(feats.data_ptr(), _DT[feats.dtype], n, feats.stride(0), d, text.data_ptr(), q, text.stride(0),
                                   float(scale), _NORM[normalize], out.data_ptr(), _DT[out.dtype], out.stride(0), ws.data_ptr(), wsb,
                                   stream)
    else:
        if e == _abi.SAF_QW_ROW_ARGMAX:
            idx = torch.full((n,), -7, dtype=torch.int32, device=dev)
            val = torch.full((n,), float("nan"), device=dev)
        elif e == _abi.SAF_QW_QUERY_MAX:
            val = torch.full((q,), float("nan"), device=dev)
            row = torch.full((q,), -7, dtype=torch.int64, device=dev)
        wsb = L.saf_query_wide_ex_workspace_bytes(q, d, e, n_bg)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        assert ws.data_ptr() % 256 == 0
        rc = L.saf_query_scan_wide_ex(feats.data_ptr(), _DT[feats.dtype], n, feats.stride(0), d, text.data_ptr(), q, text.stride(0),
                                      float(scale), _NORM[normalize], e, n_bg, int(rescale), _abi.ptr(out),
                                      _DT[out.dtype] if out is not None else _abi.SAF_F32, out.stride(0) if out is not None else 0,
                                      _abi.ptr(idx), _abi.ptr(val), _abi.ptr(row), row_offset, ws.data_ptr(), wsb, stream)
    torch.cuda.synchronize()
    assert rc == 0, f"rc {rc}: {L.saf_last_error().decode()}"
    if out is not None:
        return out
    return (idx, val) if idx is not None else (val, row)


def _padded(t, pad):
    """`t` as the [:, :D] view of a [rows, D + pad] device tensor whose other columns are NaN"""
    wide = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype)
    wide[:, : t.shape[1]] = t
    view = wide.cuda()[:, : t.shape[1]]
    assert view.stride(0) == t.shape[1] + pad and not view.is_contiguous() and view.data_ptr() % 16 == 0
    return view


@functools.lru_cache(maxsize=None)
def _scene(n, d, q, dt, seed=0):
    """randn rows in `dt` with an all-zero row, two tied rows and a row every query scores below zero (the zero-padded columns of the
    last tile would win its argmax); unit text rows with two tied queries.  Cached: nobody writes to it."""
    g = torch.Generator().manual_seed(977 * n + 31 * d + q + seed)
    text = torch.nn.functional.normalize(torch.randn(q, d, generator=g), dim=-1)
    if q > 20:
        text[17] = text[5]  # tied queries: the first one wins a row's argmax
    feats = torch.randn(n, d, generator=g)
    feats[min(77, n - 1)] = 0
    if n > 300:
        feats[229] = feats[100]  # tied rows (another lane, another register): the first one wins a query's maximum
        feats[300] = -(torch.linalg.pinv(text.double()) @ torch.ones(q, dtype=torch.float64)).float()  # <f, t_q> = -1 for every q
    return feats.to(dt), text


@functools.lru_cache(maxsize=None)
def _truth(oracle, n, d, q, dt, seed=0):
    feats, text = _scene(n, d, q, dt, seed)
    s = oracle.wide_scan(feats, text, "scores", round_to=dt)
    vb = oracle.wide_scan(feats, text, "vs_background", scale=100.0, n_background=N_BG, round_to=dt)
    return s, vb


def _check_reductions(s, ra, qm, what, row_offset=0):
    """ROW_ARGMAX (idx, val) and QUERY_MAX (val, row) against the oracle's scores `s` (finite)"""
    n, q = s.shape
    idx, val = ra[0].cpu().long(), ra[1].cpu()
    assert bool(((idx >= 0) & (idx < q)).all()), f"{what}: a row's best query is outside [0, {q})"
    best = s.max(dim=1).values
    e_val, e_pick = (val - best).abs().max().item(), (s[torch.arange(n), idx] - best).abs().max().item()
    qv, qr = qm[0].cpu(), qm[1].cpu() - row_offset
    assert bool(((qr >= 0) & (qr < n)).all()), f"{what}: a query's best row is outside [0, {n})"
    qbest = s.max(dim=0).values
    e_qv, e_qpick = (qv - qbest).abs().max().item(), (s[qr, torch.arange(q)] - qbest).abs().max().item()
    print(f"{what}: row_argmax value err {e_val:.3g}, its query's score below the best by {e_pick:.3g}; query_max value err {e_qv:.3g}, "
          f"its row's score below the best by {e_qpick:.3g}")
    assert e_val <= VAL and e_pick <= VAL, f"{what}: row_argmax"
    assert e_qv <= VAL and e_qpick <= VAL, f"{what}: query_max"
    return idx, qr


# ---------------------------------------------------------------------------------------------------------------------------
# A. strides
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("pad", [8, 72])
@pytest.mark.parametrize("q", [33, 96])
@pytest.mark.parametrize("d,dt", [(256, F16), (512, F16), (256, BF16), (512, BF16)], ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_strided_rows_and_text(oracle, monkeypatch, form, pad, q, d, dt):
    """feats as the [:, :D] view of [n, D + 8] / [n, D + 72] and text as the [:, :D] view of [Q, D + 24], the other columns NaN:
    777 rows (three 256-row blocks and a ragged one), every epilogue: each result equals the contiguous call's bit for bit and the
    oracle within the bar of its output type (16-bit out with pad 8, fp32 out with pad 72)."""
    from spatially_aware_ai_amd.clipfusion import query_scan_wide

    monkeypatch.setenv("SAF_WIDE_MFMA", form)
    n = 777
    feats, text = _scene(n, d, q, dt)
    s, vb = _truth(oracle, n, d, q, dt)
    fv, tv = _padded(feats, pad), _padded(text, 24)
    fc, tc = feats.cuda(), text.cuda()
    odt = dt if pad == 8 else F32
    what = f"form {form}, D {d}, {_name(dt)}, Q {q}, feat_stride {d + pad}"
    for epi, kw, want, tol in (("scores", {}, s, TOL[odt]), ("vs_background", dict(scale=100.0, n_bg=N_BG), vb, max(TOL[odt], 2e-3))):
        got = _wide(fv, tv, epi, out_dtype=odt, **kw)
        ref = query_scan_wide(fc, tc, epi, out_dtype=odt, scale=kw.get("scale", 1.0), n_background=kw.get("n_bg", 0))
        err = (got.float().cpu() - want).abs().max().item()
        print(f"{what}: {epi} max abs err {err:.3g}")
        assert _same_bits(got, ref), f"{what}: {epi} differs from the contiguous call"
        assert err <= tol, f"{what}: {epi} max abs err {err}"
    assert float(got.float().abs().max()) <= 1.0
    ra, qm = _wide(fv, tv, "row_argmax"), _wide(fv, tv, "query_max", row_offset=5000)
    for a, b in zip(ra + qm, query_scan_wide(fc, tc, "row_argmax") + query_scan_wide(fc, tc, "query_max", row_offset=5000)):
        assert _same_bits(a, b), f"{what}: a reduction differs from the contiguous call"
    idx, qr = _check_reductions(s, ra, qm, what, row_offset=5000)
    assert int(idx[77]) == 0 and float(ra[1][77]) == 0.0, "the all-zero row: every query ties at 0, the first one wins"
    assert float(s[300].max()) < 0 and float(ra[1][300]) < 0, "the row every query scores below zero: no zero-padded column may win"
    if q > 20:
        assert not bool((idx == 17).any()), "of two tied queries the first must win"
    assert not bool((qr == 229).any()), "of two tied rows the first must win"


@pytest.mark.parametrize("pad", [8, 72])
@pytest.mark.parametrize("q", [64, 203])
@pytest.mark.parametrize("dt", [F16, BF16], ids=_name)
def test_strided_rows_and_text_first_kernel(oracle, pad, q, dt):
    """the same views at D = 128 through saf_query_scan_wide (query_wide_kernel)"""
    from spatially_aware_ai_amd.clipfusion import query_scan_wide

    n, d = 777, 128
    feats, text = _scene(n, d, q, dt)
    want = oracle.wide_scan(feats, text, "scores", round_to=dt)
    odt = dt if pad == 8 else F32
    got = _wide(_padded(feats, pad), _padded(text, 24), "scores", out_dtype=odt)
    err = (got.float().cpu() - want).abs().max().item()
    print(f"D 128, {_name(dt)}, Q {q}, feat_stride {d + pad}: max abs err {err:.3g}")
    assert _same_bits(got, query_scan_wide(feats.cuda(), text.cuda(), "scores", out_dtype=odt)), "differs from the contiguous call"
    assert err <= TOL[odt]


WRAP_N = 70001  # more than 256 row blocks of 256: one workgroup per CU, so a workgroup owns at least two blocks -- the prefetch runs


@functools.lru_cache(maxsize=None)
def _wrap_scene(dt):
    g = torch.Generator().manual_seed(70001)
    feats = (torch.randn(WRAP_N, 512, generator=g) * (0.25 + torch.rand(WRAP_N, 1, generator=g))).to(dt)
    text = torch.nn.functional.normalize(torch.randn(450, 512, generator=g), dim=-1)
    rows = torch.cat([torch.arange(0, 64), torch.linspace(64, WRAP_N - 301, 200).long(), torch.arange(WRAP_N - 300, WRAP_N)]).unique()
    return feats, text, rows  # (host tensors: the two 73 MB device copies live for one test only)


@functools.lru_cache(maxsize=None)
def _wrap_truth(oracle, dt):
    feats, text, rows = _wrap_scene(dt)
    return oracle.wide_scan(feats[rows], text, "scores", round_to=dt)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("q,dt", [(64, F16), (450, F16), (64, BF16)], ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_strided_rows_through_the_row_block_prefetch(oracle, monkeypatch, form, q, dt):
    """feat_stride = 520 over 70 001 rows of D = 512: every workgroup of query_wide3_kernel owns two row blocks and fetches the second
    one's first eleven KiB per wave through the LDS from `feats + row * feat_stride`.  Q = 64: two tiles per block, fewer than the
    prefetch has pieces (the draining wait at the block change); Q = 450: fifteen tiles, all eleven pieces, the counted wait.  SCORES
    (16-bit out) and QUERY_MAX equal the contiguous call bit for bit; the oracle is asked about 564 rows (the first 64, the last 300,
    200 between) and about the winners' rows."""
    from spatially_aware_ai_amd.clipfusion import query_scan_wide

    monkeypatch.setenv("SAF_WIDE_MFMA", form)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus * 256 < WRAP_N, f"{cus} CUs: no workgroup would own a second row block, the prefetch would not run; raise WRAP_N"
    feats, text, rows = _wrap_scene(dt)
    fv, fc = _padded(feats, 8), feats.cuda()
    text = text[:q]
    want = _wrap_truth(oracle, dt)[:, :q]
    tv, tc = _padded(text, 24), text.cuda()
    what = f"form {form}, {_name(dt)}, Q {q}, 70001 rows at stride 520"
    got = _wide(fv, tv, "scores")
    assert _same_bits(got, query_scan_wide(fc, tc, "scores")), f"{what}: scores differ from the contiguous call"
    err = (got[rows.cuda()].float().cpu() - want).abs().max().item()
    qv, qr = _wide(fv, tv, "query_max")
    rv, rr = query_scan_wide(fc, tc, "query_max")
    assert _same_bits(qv, rv) and torch.equal(qr, rr), f"{what}: query_max differs from the contiguous call"
    win = oracle.wide_scan(feats[qr.cpu()], text, "scores", round_to=dt)[torch.arange(q), torch.arange(q)]
    e_win = (win - qv.cpu()).abs().max().item()
    short = (want.max(dim=0).values - qv.cpu()).max().item()
    print(f"{what}: scores max abs err on the sampled rows {err:.3g}; query_max: winner's oracle score off by {e_win:.3g}, "
          f"below the sampled rows' best by {short:.3g}")
    assert err <= TOL[dt], f"{what}: scores"
    assert e_win <= VAL, f"{what}: a per-query winner does not have the score reported for it"
    assert short <= VAL, f"{what}: a per-query maximum is below a score that exists"


# ---------------------------------------------------------------------------------------------------------------------------
# B. output layout
# ---------------------------------------------------------------------------------------------------------------------------
SENTINEL = 0xC3  # every byte of the caller's buffer before the call


def _layouts(cols, esz):
    """(name, row stride, first element of the view in the buffer) -- in elements"""
    up = lambda v, m: (v + m - 1) // m * m
    line = 128 // esz
    s8 = up(cols, 8)
    if (s8 * esz) % 128 == 0:
        s8 += 8
    return [("odd stride: scalar stores", cols + 1, 0),
            ("stride a multiple of 8, no whole lines: vector stores", s8, 0),
            ("whole 128-byte lines", up(cols, line), 0),
            ("base one element off: scalar stores", up(cols + 1, 8), 1),
            ("base on 16 bytes, not on a line", up(cols + 16 // esz, line), 16 // esz)]


def _sentinel_view(n, cols, stride, first, dt):
    esz = torch.empty((), dtype=dt).element_size()
    buf = torch.full(((n * stride + first + 64) * esz,), SENTINEL, dtype=torch.uint8, device="cuda")  # (64 elements behind the last row)
    assert buf.data_ptr() % 128 == 0
    flat = buf.view(dt)
    view = flat[first: first + n * stride].view(n, stride)[:, :cols]
    inside = torch.zeros(flat.shape, dtype=torch.bool, device="cuda")
    inside[first: first + n * stride].view(n, stride)[:, :cols] = True
    return buf, view, inside


def _outside_untouched(buf, inside, dt):
    ints = buf.view(_BITS[torch.empty((), dtype=dt).element_size()])
    want = ints.new_tensor(int.from_bytes(bytes([SENTINEL]) * ints.element_size(), "little", signed=True))
    return bool((ints[~inside] == want).all())


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("odt", [F32, F16, BF16], ids=_name)
@pytest.mark.parametrize("epi", ["scores", "vs_background"])
@pytest.mark.parametrize("q,d,dt", [(100, 512, F16), (33, 256, BF16)], ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_caller_output_layouts(oracle, monkeypatch, form, odt, epi, q, d, dt):
    """`out` as a view into a larger buffer of sentinel bytes, five layouts (_layouts): the view equals the wrapper-allocated result bit
    for bit -- which is held to the oracle here --, every byte of the buffer outside the view still holds the sentinel, and
    query_scan_wide(..., out=view) does the same."""
    from spatially_aware_ai_amd.clipfusion import query_scan_wide

    monkeypatch.setenv("SAF_WIDE_MFMA", form)
    n = 777
    feats, text = _scene(n, d, q, dt)
    s, vb = _truth(oracle, n, d, q, dt)
    fc, tc = feats.cuda(), text.cuda()
    kw = dict(scale=100.0, n_bg=N_BG) if epi == "vs_background" else {}
    wkw = dict(scale=kw.get("scale", 1.0), n_background=kw.get("n_bg", 0))
    cols = q - kw.get("n_bg", 0)
    ref = query_scan_wide(fc, tc, epi, out_dtype=odt, **wkw)
    err = (ref.float().cpu() - (vb if epi == "vs_background" else s)).abs().max().item()
    assert err <= (max(TOL[odt], 2e-3) if epi == "vs_background" else TOL[odt]), err
    for name, stride, first in _layouts(cols, ref.element_size()):
        what = f"form {form}, {epi}, {_name(odt)} out, {cols} columns, {name} (stride {stride}, first element {first})"
        for through_wrapper in (False, True):
            buf, view, inside = _sentinel_view(n, cols, stride, first, odt)
            if through_wrapper:
                got = query_scan_wide(fc, tc, epi, out=view, **wkw)
                torch.cuda.synchronize()
                assert got.data_ptr() == view.data_ptr() and got.stride() == view.stride()
            else:
                got = _wide(fc, tc, epi, out=view, **kw)
            assert _same_bits(view, ref), f"{what}: differs from the wrapper-allocated result (out= of query_scan_wide: {through_wrapper})"
            assert _outside_untouched(buf, inside, odt), f"{what}: the scan wrote outside the view (out= of query_scan_wide: {through_wrapper})"


@pytest.mark.parametrize("odt", [F32, F16, BF16], ids=_name)
@pytest.mark.parametrize("q,dt", [(100, F16), (33, BF16)], ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_caller_output_layouts_first_kernel(oracle, odt, q, dt):
    """the same layouts at D = 128 through saf_query_scan_wide, whose kernel picks its store route by a rule of its own (a stride that
    is a multiple of 4 and a base on 16 bytes); `cols` itself as the stride when it is a multiple of 4"""
    from spatially_aware_ai_amd.clipfusion import query_scan_wide

    n, d = 777, 128
    feats, text = _scene(n, d, q, dt)
    fc, tc = feats.cuda(), text.cuda()
    ref = query_scan_wide(fc, tc, "scores", out_dtype=odt)
    err = (ref.float().cpu() - oracle.wide_scan(feats, text, "scores", round_to=dt)).abs().max().item()
    assert err <= TOL[odt], err
    layouts = _layouts(q, ref.element_size()) + [("stride a multiple of 4 only", (q + 3) // 4 * 4 + (4 if (q + 3) // 4 % 2 == 0 else 0), 0)]
    for name, stride, first in layouts:
        what = f"D 128, {_name(odt)} out, {q} columns, {name} (stride {stride}, first element {first})"
        for through_wrapper in (False, True):
            buf, view, inside = _sentinel_view(n, q, stride, first, odt)
            if through_wrapper:
                got = query_scan_wide(fc, tc, "scores", out=view)
                torch.cuda.synchronize()
                assert got.data_ptr() == view.data_ptr() and got.stride() == view.stride()
            else:
                _wide(fc, tc, "scores", out=view)
            assert _same_bits(view, ref), f"{what}: differs from the wrapper-allocated result (out= of query_scan_wide: {through_wrapper})"
            assert _outside_untouched(buf, inside, odt), f"{what}: the scan wrote outside the view (out= of query_scan_wide: {through_wrapper})"


# ---------------------------------------------------------------------------------------------------------------------------
# C. non-finite and extreme rows
# ---------------------------------------------------------------------------------------------------------------------------
INF, NAN = float("inf"), float("nan")
# of a wave's 32 rows: 0, 4 and 16 head a chain of the interleaved per-query maximum in one form or the other; 1, 5 and 31 do not
OFFSETS = (0, 4, 16, 1, 5, 31)


def _plant(feats, n):
    """five kinds of bad row -- one +inf, one -inf, one NaN, all +inf, inf and NaN together -- at OFFSETS of a wave's rows in two
    interior 256-row blocks (each kind at a chain head and elsewhere), in the first wave of the scan, and in the last wave, which is
    ragged at n = 1000 (rows 992..999).  Returns the bad rows."""
    d = feats.shape[1]
    kinds = [lambda r: r.__setitem__(17, INF), lambda r: r.__setitem__(d - 1, -INF), lambda r: r.__setitem__(d // 2, NAN),
             lambda r: r.fill_(INF), lambda r: (r.__setitem__(3, INF), r.__setitem__(min(200, d - 2), NAN))]
    rows = [256 + 64 + o for o in OFFSETS] + [512 + 160 + o for o in OFFSETS] + [0, 4] + [992 + o for o in (0, 4, 1, 5)]
    for i, row in enumerate(rows):
        assert row < n
        kinds[(i + i // 6) % 5](feats[row])
    return torch.tensor(rows)


@functools.lru_cache(maxsize=None)
def _bad_scene(oracle, n, d, dt):
    g = torch.Generator().manual_seed(n + d)
    good = torch.randn(n, d, generator=g).to(dt)
    text = torch.nn.functional.normalize(torch.randn(96, d, generator=g), dim=-1)
    bad = good.clone()
    rows = _plant(bad, n)
    is_bad = torch.zeros(n, dtype=torch.bool)
    is_bad[rows] = True
    want = {m: oracle.wide_scan(bad, text, "scores", normalize=_ONORM[m], round_to=dt) for m in (True, False, "clamp")}
    return good.cuda(), bad.cuda(), text.cuda(), is_bad, want


def _check_bad_scores(what, s_good, s_bad, want, is_bad, normalize):
    """fp32 scores of the volume with (`s_bad`) and without (`s_good`) the bad rows against the oracle's of the volume with them"""
    assert torch.equal(_bits(s_bad[~is_bad]), _bits(s_good[~is_bad])), f"{what}: a bad row changed a good row's scores"
    err = (s_bad[~is_bad] - want[~is_bad]).abs().max().item()
    print(f"{what}: good rows' scores max abs err {err:.3g}")
    assert err <= TOL[F32], f"{what}: good rows' scores"
    gb, wb = s_bad[is_bad], want[is_bad]
    if normalize is True:
        assert bool((wb == 0).all()) and bool((gb == 0).all()), f"{what}: a bad row must score 0 in every column"
    else:
        assert not bool(torch.isfinite(wb).any()), "the oracle's scores of a bad row are not finite without nan_to_num"
        assert torch.equal(torch.isnan(gb), torch.isnan(wb)), f"{what}: NaN scores where the oracle has none, or the reverse"
        assert torch.equal(gb[~torch.isnan(wb)], wb[~torch.isnan(wb)]), f"{what}: infinite scores differ from the oracle's"


@pytest.mark.parametrize("normalize", [True, False, "clamp"], ids=["l2", "raw", "clamp"])
@pytest.mark.parametrize("n", [1024, 1000])
@pytest.mark.parametrize("d,dt", [(128, BF16), (128, F16), (512, F16)], ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_rows_with_inf_and_nan_first_kernel(oracle, normalize, n, d, dt):
    """the same rows through saf_query_scan_wide (query_wide_kernel, D = 128 and D = 512), which include/saf.h holds to the same rules:
    a bad row scores exactly 0 in every column under normalize=True; raw and under "clamp" its scores are NaN / the same infinity
    where the oracle's are; every good row is bit for bit what it is without the bad rows, and within 3e-5 of the oracle."""
    good, bad, text, is_bad, want_all = _bad_scene(oracle, n, d, dt)
    what = f"first kernel, D {d}, {_name(dt)}, {n} rows, normalize={normalize}"
    s_good = _wide(good, text, "scores", normalize=normalize, out_dtype=F32, first=True).cpu()
    s_bad = _wide(bad, text, "scores", normalize=normalize, out_dtype=F32, first=True).cpu()
    _check_bad_scores(what, s_good, s_bad, want_all[normalize], is_bad, normalize)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("normalize", [True, False, "clamp"], ids=["l2", "raw", "clamp"])
@pytest.mark.parametrize("n", [1024, 1000])
@pytest.mark.parametrize("d,dt", [(512, F16), (256, BF16)], ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_rows_with_inf_and_nan(oracle, monkeypatch, form, normalize, n, d, dt):
    """Rows with an inf or a NaN in them, as fp16 fusion can leave them (tests/test_fp16_volume_gpu.py), among good rows.

    SCORES: under normalize=True a bad row scores exactly 0 in every column (nan_to_num: the all-zero row), as the oracle says; raw
    and under "clamp" its scores are NaN where the oracle's are and the same infinity where the oracle's are infinite.  Every good
    row's scores equal, bit for bit, the scan of the volume without the bad rows, and the oracle within 3e-5.
    ROW_ARGMAX: a good row's index and value are unchanged bit for bit; a bad row's index lies in [0, Q) and under normalize=True it
    is index 0, value 0.
    QUERY_MAX: the oracle's per-query maximum over the scores that are not NaN, the first row among equals (several rows score +inf
    for one query when unnormalised); an infinite score is a score and wins; a NaN never does, wherever its row sits.

    Measured on an MI355X, the worst of both forms, both shapes and both row counts -- good rows' scores against the oracle: 7.5e-8
    normalised and under "clamp", 1.7e-6 raw (scores of size 1..4); QUERY_MAX values against the oracle's: 6.7e-8 normalised and
    under "clamp", 9.5e-7 raw; the winner's own oracle score below the oracle's best: 0 in all 24 cases."""
    monkeypatch.setenv("SAF_WIDE_MFMA", form)
    good, bad, text, is_bad, want_all = _bad_scene(oracle, n, d, dt)
    want = want_all[normalize]
    q = text.shape[0]
    what = f"form {form}, D {d}, {_name(dt)}, {n} rows, normalize={normalize}"
    s_good = _wide(good, text, "scores", normalize=normalize, out_dtype=F32).cpu()
    s_bad = _wide(bad, text, "scores", normalize=normalize, out_dtype=F32).cpu()
    _check_bad_scores(what, s_good, s_bad, want, is_bad, normalize)
    # per-row argmax
    ig, vg = _wide(good, text, "row_argmax", normalize=normalize)
    ib, vb = _wide(bad, text, "row_argmax", normalize=normalize)
    ig, vg, ib, vb = ig.cpu(), vg.cpu(), ib.cpu(), vb.cpu()
    assert torch.equal(ib[~is_bad], ig[~is_bad]) and torch.equal(_bits(vb[~is_bad]), _bits(vg[~is_bad])), f"{what}: a good row's argmax changed"
    assert bool(((ib >= 0) & (ib < q)).all()), f"{what}: a row's best query is outside [0, {q})"
    if normalize is True:
        assert bool((ib[is_bad] == 0).all()) and bool((vb[is_bad] == 0).all()), f"{what}: a bad row's argmax is not (0, 0.0)"
    # per-query maximum over the scores that are not NaN
    qv, qr = _wide(bad, text, "query_max", normalize=normalize)
    qv, qr = qv.cpu(), qr.cpu()
    live = torch.where(torch.isnan(want), torch.full_like(want, -INF), want)
    best = live.max(dim=0).values
    assert not bool(torch.isnan(qv).any()), f"{what}: a NaN won a query's maximum"
    assert bool(((qr >= 0) & (qr < n)).all())
    picked = live[qr, torch.arange(q)]
    infinite = torch.isinf(best)
    assert torch.equal(qv[infinite], best[infinite]) and torch.equal(picked[infinite], best[infinite]), f"{what}: an infinite score must win"
    first = torch.argmax((live == best[None]).int(), dim=0)
    assert torch.equal(qr[infinite], first[infinite]), f"{what}: of equal (infinite) scores the first row must win"
    if bool((~infinite).any()):
        e_v, e_p = (qv - best)[~infinite].abs().max().item(), (picked - best)[~infinite].abs().max().item()
        print(f"{what}: query_max value err {e_v:.3g}, its row's score below the best by {e_p:.3g}")
        assert e_v <= VAL and e_p <= VAL, f"{what}: query_max is not the maximum over the scores that are not NaN"
    if normalize is True:
        # heat maps of a bad row: the all-zero row's, 1 / (1 + number of backgrounds)
        hm = _wide(bad, text, "vs_background", scale=100.0, n_bg=N_BG, out_dtype=F32).cpu()
        assert bool((hm[is_bad] == hm[is_bad][0, 0]).all()) and abs(float(hm[is_bad][0, 0]) - 1.0 / (1 + N_BG)) <= 2e-3


# raw scores: |score - float64| <= RAW_REL * sum_k |f_k t_k|.  What test_rows_of_any_magnitude measures against float64 on an MI355X plus
# one fp32 ulp (2^-24): fp16, D = 512: 21.364 x 2^-24; bf16, D = 256: 1.461 x 2^-24.  The fp16 figure comes from four rows only, the
# smallest of the rows at one power of ten each: every element a subnormal of 1..18 x 2^-24 (max |f| 3e-7 .. 1e-6), 390-460 of them
# non-zero.  Their absolute error is the same 1.6e-12 .. 2.0e-12 (about 2^-39) whatever the row's size, so relative to the smallest
# row's sum |f t| = 1.4e-6 it is 21 x 2^-24 and falls to 13, 11 and 6 in the next three rows: the matrix instruction drops what a
# product of a subnormal fp16 operand has below about 2^-40, a floor in absolute terms.  With the subnormal elements zeroed the same
# rows measure 1.2 x 2^-24; every other block measures 1.1 .. 1.9 (subnormals of 1e-5, rows of 65504, every second element 0).  So
# the constant guards ordinary rows loosely and those four rows tightly.  (The narrow scan's bound in tests/test_split_scan.py,
# CUT + ACC_WORST, is 112 x 2^-24.)
RAW_REL = {F16: 22.364 * 2.0 ** -24, BF16: 2.461 * 2.0 ** -24}


def _magnitude_rows(dt, d, g):
    blocks = []
    base = lambda: torch.randn(64, d, generator=g)
    if dt == F16:
        blocks.append(base() * 1.0e-5)                                       # fp16 subnormals only (below 6.1e-5), some flushed to 0
        blocks.append(torch.sign(base()) * 65504.0)                         # the largest finite fp16 in every element
        blocks.append(base() * torch.logspace(-7, 4, 64)[:, None])          # one power of ten per row, subnormal to 4 sigma below 65504
    else:
        blocks.append(base() * torch.logspace(-15, 15, 64)[:, None])        # bf16: as far as an fp32 sum of squares holds
    half = base()
    half[:, ::2] = 0.0                                                      # every second element 0
    blocks.append(half)
    last = torch.zeros(64, d)
    last[:, -1] = torch.randn(64, generator=g) * 3.0                        # a single non-zero element, the last
    blocks.append(last)
    rows = torch.cat(blocks).to(dt)
    assert bool(torch.isfinite(rows.float()).all()) and bool((rows.float().abs().sum(dim=1) > 0).all())
    if dt == F16:
        assert float(rows[:64].float().abs().max()) < 2.0 ** -14
    return rows


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("d,dt", [(512, F16), (256, BF16)], ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_rows_of_any_magnitude(oracle, monkeypatch, form, d, dt):
    """Finite rows at the ends of what the dtype and an fp32 sum of squares hold, in blocks of 64 (_magnitude_rows), 96 unit queries.
    Normalised scores against the oracle at 3e-5; raw scores (normalize=False, fp32 out) against float64 of the same 16-bit operands
    within RAW_REL of sum_k |f_k t_k| per score, the form of bound tests/test_split_scan.py states for the narrow scan (there with the
    cut's term, which this scan does not have: its products of 16-bit operands are exact); the constant is the measured one, see
    RAW_REL.  Measured on an MI355X, both forms alike: normalised scores against the oracle 8.2e-7 (fp16, the rows at one power of
    ten each; 6e-8 elsewhere) and 6e-8 (bf16); raw scores 21.364 x 2^-24 (fp16) and 1.461 x 2^-24 (bf16) of sum |f t|."""
    monkeypatch.setenv("SAF_WIDE_MFMA", form)
    g = torch.Generator().manual_seed(4 * d)
    rows = _magnitude_rows(dt, d, g)
    text = torch.nn.functional.normalize(torch.randn(96, d, generator=g), dim=-1)
    fd, td = rows.cuda(), text.cuda()
    what = f"form {form}, D {d}, {_name(dt)}"
    want = oracle.wide_scan(rows, text, "scores", round_to=dt)
    got = _wide(fd, td, "scores", out_dtype=F32).cpu()
    err = (got - want).abs()
    print(f"{what}: normalised scores max abs err {err.max().item():.3g} (per block of 64 rows: "
          f"{[float(f'{e:.2g}') for e in err.view(-1, 64, 96).amax(dim=(1, 2)).tolist()]})")
    raw = _wide(fd, td, "scores", normalize=False, out_dtype=F32).double().cpu().numpy()
    f64, t64 = rows.double().numpy(), text.to(dt).double().numpy()
    mag = np.abs(f64) @ np.abs(t64).T
    rel = np.abs(raw - f64 @ t64.T) / np.where(mag > 0, mag, 1.0)
    print(f"{what}: raw scores max err / sum |f t| = {rel.max():.4g} = {rel.max() * 2.0 ** 24:.3f} x 2^-24 (per block: "
          f"{[float(f'{e:.2g}') for e in rel.reshape(-1, 64 * 96).max(axis=1) * 2.0 ** 24]} x 2^-24)")
    assert err.max().item() <= TOL[F32], f"{what}: normalised scores"
    assert (rel <= RAW_REL[dt]).all(), f"{what}: raw scores off by {rel.max() * 2.0 ** 24:.3f} x 2^-24 of sum |f t|"
    # the reductions see the same rows
    _check_reductions(want, _wide(fd, td, "row_argmax"), _wide(fd, td, "query_max"), what)


# ---------------------------------------------------------------------------------------------------------------------------
# D. reductions without L2 normalisation, and the per-query maximum under a negative scale
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed_norms(n, d, dt):
    g = torch.Generator().manual_seed(n + 3 * d)
    feats = torch.randn(n, d, generator=g)
    feats[: n // 2] *= 0.001  # norms below 0.1: "clamp" divides by 0.1, not by the norm
    text = torch.nn.functional.normalize(torch.randn(96, d, generator=g), dim=-1)
    return feats.to(dt), text


MODES = [(False, 1.0), ("clamp", 1.0), (True, -2.0), (False, -2.0)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("d,dt", [(512, F16), (256, BF16)], ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_reductions_under_other_modes(oracle, monkeypatch, form, d, dt):
    """ROW_ARGMAX and QUERY_MAX raw and under "clamp", over rows half of which have norms below 0.1 -- QUERY_MAX compares each row's
    product times that row's factor, so the factor decides the winner --, and both under scale = -2 (the best is the smallest
    cosine): 777 rows against the oracle's reductions of its own scores."""
    monkeypatch.setenv("SAF_WIDE_MFMA", form)
    feats, text = _mixed_norms(777, d, dt)
    fd, td = feats.cuda(), text.cuda()
    for normalize, scale in MODES:
        s = oracle.wide_scan(feats, text, "scores", scale=scale, normalize=_ONORM[normalize], round_to=dt)
        ra = _wide(fd, td, "row_argmax", scale=scale, normalize=normalize)
        qm = _wide(fd, td, "query_max", scale=scale, normalize=normalize)
        _, qr = _check_reductions(s, ra, qm, f"form {form}, D {d}, {_name(dt)}, 777 rows, normalize={normalize}, scale={scale}")
        if normalize is not True:
            assert bool((qr >= 777 // 2).all()), "a row a thousand times shorter cannot win unnormalised"


@pytest.mark.parametrize("form", FORMS)
def test_reductions_under_other_modes_over_many_blocks(oracle, monkeypatch, form):
    """the same over 70 000 fp16 rows of D = 512 (every workgroup wraps to a second row block).  QUERY_MAX: the winners' rows are
    gathered and scored by the oracle (each must have the value reported for it), and no row of a float64 matrix product on the
    device scores higher; ROW_ARGMAX: 564 sampled rows against the oracle."""
    monkeypatch.setenv("SAF_WIDE_MFMA", form)
    n, d, dt = 70000, 512, F16
    feats, text = _mixed_norms(n, d, dt)
    fd, td = feats.cuda(), text.cuda()
    q = text.shape[0]
    rows = torch.cat([torch.arange(0, 64), torch.linspace(64, n - 301, 200).long(), torch.arange(n - 300, n)]).unique()
    t64 = text.to(dt).double().cuda()
    for normalize, scale in MODES:
        what = f"form {form}, 70000 rows, normalize={normalize}, scale={scale}"
        qv, qr = _wide(fd, td, "query_max", scale=scale, normalize=normalize)
        qv, qr = qv.cpu(), qr.cpu()
        assert bool(((qr >= 0) & (qr < n)).all())
        win = oracle.wide_scan(feats[qr], text, "scores", scale=scale, normalize=_ONORM[normalize], round_to=dt)[torch.arange(q), torch.arange(q)]
        e_win = (win - qv).abs().max().item()
        best = torch.full((q,), -INF, dtype=torch.float64, device="cuda")
        for r0 in range(0, n, 10000):  # float64 on the device, 10 000 rows at a time
            f64 = fd[r0: r0 + 10000].double()
            norm = f64.norm(dim=1, keepdim=True)
            f64 = f64 / (norm.clamp_min(0.1) if normalize == "clamp" else norm) if normalize else f64
            best = torch.maximum(best, (scale * (f64 @ t64.T)).amax(dim=0))
        short = (best.cpu() - qv.double()).max().item()
        ri, rv = _wide(fd, td, "row_argmax", scale=scale, normalize=normalize)
        s = oracle.wide_scan(feats[rows], text, "scores", scale=scale, normalize=_ONORM[normalize], round_to=dt)
        ri, rv = ri.cpu()[rows].long(), rv.cpu()[rows]
        assert bool(((ri >= 0) & (ri < q)).all())
        rbest = s.max(dim=1).values
        e_rv, e_rp = (rv - rbest).abs().max().item(), (s[torch.arange(len(rows)), ri] - rbest).abs().max().item()
        print(f"{what}: query_max winner's oracle score off by {e_win:.3g}, below the float64 best by {short:.3g}; row_argmax value err "
              f"{e_rv:.3g}, its query's score below the best by {e_rp:.3g}")
        assert e_win <= VAL and short <= VAL, f"{what}: query_max"
        assert e_rv <= VAL and e_rp <= VAL, f"{what}: row_argmax"
