"""The narrow text scan (saf_query_scan, saf_query_topk) on rows that hold an inf or a NaN: what the bad-row tests share.

include/saf.h states the rule.  A row is BAD when it holds an inf or a NaN; in these tests the bad rows are exactly the planted ones.

  * SAF_NORM_L2: the reference divides the row by its norm and applies nan_to_num element by element (clip_seem_fusion.py:507-511),
    so a bad row is the all-zero row: raw score 0, softmax 1 / L, surgery 0, top-k labels 0 .. k - 1 at probability 1 / L.
  * SAF_NORM_NONE, SAF_NORM_L2_CLAMP: no nan_to_num in the reference (eval_scannet_segmentation.py:549-551 divides and goes on);
    a bad row's outputs are not finite.  Whether a value is NaN or an infinity depends on the route (the split scans cut an inf into
    hi = inf, lo = inf - inf = NaN), so only "not finite" and, where both sides are infinite, the sign are compared.
  * In every mode a good row is bit for bit what it is without the bad rows.

Here: the volumes (`scene`, `plant`), the table of routes with the dispatch conditions restated from include/saf.h and the comments of
csrc/saf_query.hip (`expected_kernels`), a float64 statement of the reference's lines in plain torch (`statement`, `stable_topk`) that
shares no code with oracle/saf_oracle.c, and ctypes callers of the C ABI (`scan`, `topk`).  tests/test_text_scan_bad_rows_host.py
holds the oracle against the statement and the rule on the CPU; tests/test_text_scan_bad_rows.py holds the HIP kernels against the
oracle and the rule.
"""
import functools

import numpy as np
import torch

from spatially_aware_ai_amd import _abi

RTOL, ATOL = 1e-4, 2e-6  # the project's tolerance on a scan's outputs (tests/test_query_outputs.py)
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
INF, NAN = float("inf"), float("nan")
POISON = -777.25  # what the output buffers hold before a call: no scan of these inputs stores it
EPILOGUES = ((_abi.SAF_Q_SCORES, 3.0), (_abi.SAF_Q_SOFTMAX, 100.0), (_abi.SAF_Q_SURGERY, 1.0))
MODES = (_abi.SAF_NORM_NONE, _abi.SAF_NORM_L2, _abi.SAF_NORM_L2_CLAMP)
MODE_NAMES = {_abi.SAF_NORM_NONE: "none", _abi.SAF_NORM_L2: "l2", _abi.SAF_NORM_L2_CLAMP: "clamp"}
N_MAIN, N_SMALL = 1000, 40  # 31 whole 32-row tiles and a ragged one of 8; one whole tile and a ragged one of 8
KIND_NAMES = ("one +inf", "one -inf", "one NaN", "all +inf", "inf and NaN")


def name(dt):
    return str(dt).split(".")[-1]


# ------------------------------------------------------------------------------------------ the volumes
def _kinds(d):
    """the five kinds of bad row of tests/test_wide_scan_edges.py's _plant, as functions that write into a row"""
    return (lambda r: r.__setitem__(17, INF), lambda r: r.__setitem__(d - 1, -INF), lambda r: r.__setitem__(d // 2, NAN),
            lambda r: r.fill_(INF), lambda r: (r.__setitem__(3, INF), r.__setitem__(min(200, d - 2), NAN)))


def bad_rows(n, row0=False):
    """[(row, kind)]: where the bad rows lie.  n = 1000: tile-local offsets 0, 1, 4, 16, 31 of tile 1 (rows 32 + o) and of an interior
    tile (512 + o), offsets 0 and 31 / 0 and 16 of two more interior tiles (256, 768), and rows 992, 996, 999 of the ragged last tile.
    The rows at offset 0 (32, 256, 512, 768, 992) are of the five kinds in turn, and every kind lies at another offset as well.
    n = 40: offsets 1, 4, 16, 31 of the whole tile and rows 32, 36, 39 of the ragged one.  Row 0 stays good (the surgery weights
    come from it) unless `row0`."""
    if n == N_MAIN:
        heads = [32, 256, 512, 768, 992]
        rest = [32 + o for o in (1, 4, 16, 31)] + [512 + o for o in (1, 4, 16, 31)] + [256 + 31, 768 + 16, 996, 999]
        rows = [(r, i) for i, r in enumerate(heads)] + [(r, (i + 2) % 5) for i, r in enumerate(rest)]
    else:
        assert n == N_SMALL
        rows = [(r, i % 5) for i, r in enumerate([32, 1, 4, 16, 31, 36, 39])]
    if row0:
        rows.append((0, 0))
    assert all(0 <= r < n for r, _ in rows) and len({r for r, _ in rows}) == len(rows)
    return rows


def plant(feats, row0=False):
    """writes the bad rows into `feats` [n, d] (any dtype: inf and NaN exist in all three); returns the bad rows' mask"""
    n, d = feats.shape
    kinds = _kinds(d)
    is_bad = torch.zeros(n, dtype=torch.bool)
    for r, k in bad_rows(n, row0):
        kinds[k](feats[r])
        is_bad[r] = True
    return is_bad


@functools.lru_cache(maxsize=None)
def scene(n, d, nl, dt, row0=False):
    """(good, bad, text, is_bad): `good` [n, d] in `dt`, `bad` the same volume with the planted rows, unit text rows [nl, d] fp32.
    Cached: nobody writes to it.

    Rows have norms around 1 (0.5 .. 1.5), so that the unnormalised scores are of a cosine's size and the project's absolute
    tolerance means under SAF_NORM_NONE what it means under SAF_NORM_L2; every fifth row is 0.08 times that (norms 0.04 .. 0.12: the
    clamp of SAF_NORM_L2_CLAMP takes hold on most of them).  No element of the normal draw is smaller than 0.1 before the row is
    scaled, which keeps every fp16 element normal (about 1.2e-4 at the least, d = 768, against 6.1e-5): what the matrix cores do
    with fp16 denormals is not this test's subject.  `row0`: row 0 is bad in `bad` and all zero in `good` (the volume whose surgery weights a bad row 0 must give)."""
    g = torch.Generator().manual_seed(7919 * d + 31 * nl + n)
    z = torch.randn((n, d), generator=g)
    z = torch.sign(z) * z.abs().clamp_min(0.1)
    size = 0.5 + torch.rand((n, 1), generator=g)
    size[4::5] *= 0.08
    good = (z / z.norm(dim=-1, keepdim=True) * size).to(dt)
    text = torch.nn.functional.normalize(torch.randn((nl, d), generator=g), dim=-1)
    bad = good.clone()
    is_bad = plant(bad, row0)
    if row0:
        good[0] = 0
    return good, bad, text, is_bad


# ------------------------------------------------------------------------------------------ the routes
# (route, D, L, dtype, padded, env): `padded` reads the rows through feat_stride = D + 8, the padding NaN; env: SAF_Q_SPLIT
ROUTES = (
    [("wave-per-row", 100, nl, dt, False, None) for nl in (5, 70) for dt in (F32, BF16, F16)]
    + [("exact", 72, 37, F32, False, None), ("exact", 512, 33, F32, False, "0")]
    + [("split", 512, nl, F32, False, None) for nl in (5, 33, 64)]
    + [("split16", 512, nl, dt, False, None) for nl in (33, 64) for dt in (F16, BF16)]
    + [("blocks-64", 512, 100, dt, False, None) for dt in (F32, F16)]
    + [("blocks-32", 768, 40, F32, False, None)]
    + [("split", 512, 33, F32, True, None), ("split16", 512, 33, BF16, True, None)]
)
# one case per route at 40 rows, and with a bad row 0 under surgery
ONE_PER_ROUTE = [("wave-per-row", 100, 70, F32, False, None), ("exact", 72, 37, F32, False, None), ("exact", 512, 33, F32, False, "0"),
                 ("split", 512, 33, F32, False, None), ("split16", 512, 64, F16, False, None), ("blocks-64", 512, 100, F32, False, None),
                 ("blocks-32", 768, 40, F32, False, None)]
# top-k: (route, D, L, dtype)
TOPK_ROUTES = [("topk-rows", 100, 20, F32), ("topk-one-block", 512, 20, F32), ("topk-one-block", 512, 64, F32),
               ("topk-carried-64", 512, 100, F32), ("topk-carried-64", 512, 100, F16), ("topk-carried-64", 512, 100, BF16),
               ("topk-carried-32", 768, 40, F32)]


def route_id(case):
    route, d, nl, dt = case[:4]
    padded, env = (case[4], case[5]) if len(case) > 4 else (False, None)
    return f"{route}-D{d}-L{nl}-{name(dt)}" + ("-padded" if padded else "") + ("-SPLIT0" if env == "0" else "")


def _matrix_ok(dt, stride, d, nl, aligned):
    """the matrix scans take the shape (include/saf.h: feat_dim % 8 == 0, up to 64 labels, rows on 16-byte boundaries; one or two
    32-label tiles of text, D + 5 floats a row, in 150 KiB of LDS)"""
    if d % 8 != 0 or nl > 64 or not aligned or stride % 4 != 0:
        return False
    return (2 if nl > 32 else 1) * 32 * (d + 5) * 4 <= 150 * 1024


def _matrix_kernel(dt, stride, d, split_env):
    if d % 16 == 0 and split_env != "0":
        return "query_split16_kernel" if dt != F32 and stride % 8 == 0 else "query_split_kernel"
    return "query_mfma_kernel"


def expected_kernels(dt, stride, d, nl, epi, out_given, aligned=True, split_env=None):
    """The kernels a saf_query_scan call launches, in order, from the documented conditions of the dispatch:
      * the matrix scan once where it takes the shape: the split scan for feat_dim % 16 == 0 (its 16-bit form for a 16-bit volume
        whose stride is a multiple of 8), SAF_Q_SPLIT=0 or feat_dim % 16 != 0 the exact-fp32 one;
      * more than 64 labels (more than 32 where two label tiles do not fit the LDS) with `out` given: one matrix scan per block of 64
        (32) labels and, for softmax and surgery, the finishing pass;
      * anything else -- feat_dim % 8 != 0, unaligned rows, out = NULL beyond a block -- one wave per row;
      * surgery first computes the weights from row 0 with the one-wave-per-row kernel, on every route."""
    head = ["query_kernel"] if epi == _abi.SAF_Q_SURGERY else []
    if _matrix_ok(dt, stride, d, nl, aligned):
        return head + [_matrix_kernel(dt, stride, d, split_env)]
    bw = 0
    if out_given:
        bw = 64 if nl > 64 and _matrix_ok(dt, stride, d, 64, aligned) else 32 if nl > 32 and _matrix_ok(dt, stride, d, 32, aligned) else 0
    if not bw:
        return head + ["query_kernel"]
    blocks = [_matrix_kernel(dt, stride, d, split_env)] * ((nl + bw - 1) // bw)
    return head + blocks + ([] if epi == _abi.SAF_Q_SCORES else ["finish_rows_kernel"])


def expected_topk_kernels(dt, stride, d, nl, aligned=True, split_env=None):
    """saf_query_topk: blocks of 64 labels on the matrix scan (32 where two label tiles do not fit), else one wave per row"""
    bw = 64 if _matrix_ok(dt, stride, d, 64, aligned) else 32 if _matrix_ok(dt, stride, d, 32, aligned) else 0
    return ["topk_rows_kernel"] if not bw else [_matrix_kernel(dt, stride, d, split_env)] * ((nl + bw - 1) // bw)


ROUTE_KERNELS = {  # what a route's name promises for an [N, L] softmax scan / a top-k
    "wave-per-row": ["query_kernel"], "exact": ["query_mfma_kernel"], "split": ["query_split_kernel"],
    "split16": ["query_split16_kernel"], "blocks-64": ["MATRIX", "MATRIX", "finish_rows_kernel"],
    "blocks-32": ["MATRIX", "MATRIX", "finish_rows_kernel"], "topk-rows": ["topk_rows_kernel"], "topk-one-block": ["MATRIX"],
    "topk-carried-64": ["MATRIX", "MATRIX"], "topk-carried-32": ["MATRIX", "MATRIX"],
}


def check_route(route, kernels):
    """the route a case is named after is the one the documented conditions give"""
    want = ROUTE_KERNELS[route]
    matrix = ("query_mfma_kernel", "query_split_kernel", "query_split16_kernel")
    ok = len(want) == len(kernels) and all(k in matrix if w == "MATRIX" else k == w for w, k in zip(want, kernels))
    assert ok, f"route {route}: the dispatch conditions give {kernels}"


# ------------------------------------------------------------------------------------------ the float64 statement
def statement(feats, text, epi, scale, mode):
    """[n, L] float64: the reference's lines on fp32 / 16-bit rows as stored, in plain torch.
    SAF_NORM_L2: clip_feat /= norm; nan_to_num (clip_seem_fusion.py:507-511); SAF_NORM_L2_CLAMP: norm.clamp_min(0.1) and no
    nan_to_num (eval_scannet_segmentation.py:549-551); SAF_Q_SOFTMAX: run_query (clipfusion.py:899-904); SAF_Q_SURGERY: the weights
    from row 0 and the scores minus their weighted mean over the labels (clipfusion.py:911-932)."""
    f, t = feats.double(), text.double()
    if mode != _abi.SAF_NORM_NONE:
        norm = f.pow(2).sum(dim=-1, keepdim=True).sqrt()
        if mode == _abi.SAF_NORM_L2_CLAMP:
            norm = norm.clamp_min(0.1)
        f = f / norm
        if mode == _abi.SAF_NORM_L2:
            f = torch.nan_to_num(f)
    s = f @ t.T
    if epi == _abi.SAF_Q_SCORES:
        return scale * s
    if epi == _abi.SAF_Q_SOFTMAX:
        return _softmax(scale * s)
    w = _softmax(2.0 * s[:1])
    w = w / w.mean(dim=-1, keepdim=True)
    sw = s * w
    return sw - sw.mean(dim=-1, keepdim=True)


def _softmax(x):
    m = x.max(dim=-1, keepdim=True).values
    e = torch.exp(x - m)
    return e / e.sum(dim=-1, keepdim=True)


def stable_topk(scores, k):
    """[n, k] labels of the k largest scores per row, best first, of equal scores the smaller label; scores must not be NaN"""
    s = torch.as_tensor(scores, dtype=torch.float64)
    assert not bool(torch.isnan(s).any())
    return torch.sort(s, dim=-1, descending=True, stable=True).indices[:, :k]


@functools.lru_cache(maxsize=None)
def truth(oracle, n, d, nl, dt, row0, epi, scale, mode):
    """the oracle's [n, L] output on the volume WITH the bad rows, as stored (16-bit values upcast).  Cached; nobody writes to it."""
    _, bad, text, _ = scene(n, d, nl, dt, row0)
    with np.errstate(all="ignore"):
        return oracle.query_scan(bad.float(), text, epi, scale=scale, normalize=mode).numpy()


def zero_row(nl, epi):
    """what the rule gives a bad row under SAF_NORM_L2: the all-zero row's output in every column"""
    return 1.0 / nl if epi == _abi.SAF_Q_SOFTMAX else 0.0


# ------------------------------------------------------------------------------------------ the C ABI
_FT = {F32: _abi.SAF_F32, BF16: _abi.SAF_BF16, F16: _abi.SAF_F16}


def on_device(stored, padded):
    """`stored` on the device; `padded`: as the [:, :D] view of an [n, D + 8] tensor whose other columns are NaN"""
    if not padded:
        return stored.cuda()
    n, d = stored.shape
    wide = torch.full((n, d + 8), NAN, dtype=stored.dtype)
    wide[:, :d] = stored
    return wide.cuda()[:, :d]


def scan(fd, text_d, epi, scale, mode, want_out=True, want_last=True):
    """saf_query_scan through ctypes: (rc, out, out_last); the outputs hold POISON before the call"""
    from spatially_aware_ai_amd._lib import lib

    L = lib()
    n, d = fd.shape
    nl = text_d.shape[0]
    out = torch.full((n, nl), POISON, device=fd.device) if want_out else None
    last = torch.full((n,), POISON, device=fd.device) if want_last else None
    wsb = L.saf_query_workspace_bytes(nl, epi)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=fd.device)
    rc = L.saf_query_scan(fd.data_ptr(), _FT[fd.dtype], n, fd.stride(0), d, text_d.data_ptr(), nl, text_d.stride(0), epi, float(scale),
                          mode, _abi.ptr(out), _abi.ptr(last), ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out, last


def topk(fd, text_d, scale, mode, k, want_prob=True):
    """saf_query_topk through ctypes: (rc, index [n, k] i32, prob [n, k] or None); the outputs hold -7 / POISON before the call"""
    from spatially_aware_ai_amd._lib import lib

    L = lib()
    n, d = fd.shape
    nl = text_d.shape[0]
    index = torch.full((n, k), -7, dtype=torch.int32, device=fd.device)
    prob = torch.full((n, k), POISON, device=fd.device) if want_prob else None
    wsb = L.saf_query_topk_workspace_bytes(n, nl, k)
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=fd.device)
    assert ws.data_ptr() % 256 == 0
    rc = L.saf_query_topk(fd.data_ptr(), _FT[fd.dtype], n, fd.stride(0), d, text_d.data_ptr(), nl, text_d.stride(0), float(scale), mode,
                          k, index.data_ptr(), _abi.ptr(prob), ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, index, prob


def bits(a):
    """fp32 values as their bit patterns: NaN compares equal to the same NaN"""
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)
