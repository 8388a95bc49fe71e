"""CPU: what saf_query_scan_wide and saf_query_scan_wide_ex refuse on the host (no GPU needed: nothing is launched).

Every call below stands in non-NULL fake pointers for device memory and must fail before it would use them, with the status
include/saf.h gives that kind of refusal (SAF_E_INVALID for a bad argument, SAF_E_UNSUPPORTED for a shape or type the scan does not
take, SAF_E_WORKSPACE for the workspace) and a saf_last_error() that names what was wrong."""
import pytest

from spatially_aware_ai_amd import _abi, _lib

P = 1 << 20  # a non-NULL stand-in for a device pointer, 256-byte aligned
INVALID, WORKSPACE, UNSUPPORTED = _abi.SAF_E_INVALID, _abi.SAF_E_WORKSPACE, _abi.SAF_E_UNSUPPORTED
SCORES, VS_BG, ROW_ARGMAX, QUERY_MAX = _abi.SAF_QW_SCORES, _abi.SAF_QW_VS_BACKGROUND, _abi.SAF_QW_ROW_ARGMAX, _abi.SAF_QW_QUERY_MAX
NAN = float("nan")


def _ex(**change):
    """saf_query_scan_wide_ex on a call that is fine except for `change`; ws_short = bytes taken off the workspace size."""
    l = _lib.lib()
    a = dict(feats=P, ft=_abi.SAF_F16, n=1000, fs=512, d=512, text=P, q=40, ts=512, scale=1.0, norm=_abi.SAF_NORM_L2, epi=SCORES,
             nbg=0, flags=0, out=P, ot=_abi.SAF_F16, os=40, idx=P, val=P, row=P, off=0, ws=P, ws_short=0)
    a.update(change)
    need = l.saf_query_wide_ex_workspace_bytes(a["q"], a["d"], a["epi"], a["nbg"] if a["epi"] == VS_BG else 0)
    rc = l.saf_query_scan_wide_ex(a["feats"], a["ft"], a["n"], a["fs"], a["d"], a["text"], a["q"], a["ts"], a["scale"], a["norm"],
                                  a["epi"], a["nbg"], a["flags"], a["out"], a["ot"], a["os"], a["idx"], a["val"], a["row"], a["off"],
                                  a["ws"], max(need, 256) - a["ws_short"], None)
    return rc, l.saf_last_error()


EX_REFUSALS = [
    ("feat_stride not a multiple of 8", dict(fs=516), INVALID, b"feat_stride a multiple of 8"),
    ("feats off 16 bytes", dict(feats=P + 8), INVALID, b"feats on 16 bytes"),
    ("feat_stride below feat_dim", dict(fs=504), INVALID, b"feat_stride 504 is below feat_dim 512"),
    ("text_stride below feat_dim", dict(ts=511), INVALID, b"text_stride 511 is below feat_dim 512"),
    ("scores: out_stride below the columns", dict(os=39), INVALID, b"out_stride >= n_text"),
    ("vs_background: out_stride below the columns", dict(epi=VS_BG, nbg=4, os=35), INVALID, b"out_stride >= n_text - n_background"),
    ("scores: no out", dict(out=None), INVALID, b"SCORES needs out"),
    ("no backgrounds", dict(epi=VS_BG, nbg=0), INVALID, b"1..32 background rows"),
    ("33 backgrounds", dict(epi=VS_BG, nbg=33), INVALID, b"1..32 background rows"),
    ("backgrounds only", dict(epi=VS_BG, nbg=32, q=32), INVALID, b"at least one target"),
    ("vs_background: scale 0", dict(epi=VS_BG, nbg=4, scale=0.0), INVALID, b"positive scale"),
    ("vs_background: scale < 0", dict(epi=VS_BG, nbg=4, scale=-100.0), INVALID, b"positive scale"),
    ("vs_background: scale NaN", dict(epi=VS_BG, nbg=4, scale=NAN), INVALID, b"positive scale"),
    ("row_argmax: no out_index", dict(epi=ROW_ARGMAX, idx=None), INVALID, b"out_index"),
    ("row_argmax: no out_value", dict(epi=ROW_ARGMAX, val=None), INVALID, b"out_value"),
    ("query_max: no out_value", dict(epi=QUERY_MAX, val=None), INVALID, b"out_value"),
    ("query_max: no out_row", dict(epi=QUERY_MAX, row=None), INVALID, b"out_row"),
    ("query_max: rows index past 2^32 - 1", dict(epi=QUERY_MAX, off=(1 << 32) - 1000), UNSUPPORTED, b"below 2^32"),
    ("query_max: a negative row offset", dict(epi=QUERY_MAX, off=-1), UNSUPPORTED, b"below 2^32"),
    ("feat_dim 128", dict(d=128, fs=128, ts=128), UNSUPPORTED, b"feat_dim must be 256 or 512 (got 128)"),
    ("feat_dim 384", dict(d=384, fs=384, ts=384), UNSUPPORTED, b"feat_dim must be 256 or 512 (got 384)"),
    ("bad epilogue", dict(epi=4), INVALID, b"bad epilogue 4"),
    ("negative epilogue", dict(epi=-1), INVALID, b"bad epilogue -1"),
    ("no workspace", dict(ws=None), WORKSPACE, b"workspace needs"),
    ("workspace off 256 bytes", dict(ws=P + 128), WORKSPACE, b"256-byte aligned"),
    ("workspace one byte short", dict(ws_short=1), WORKSPACE, b"workspace needs"),
    ("query_max: workspace one byte short", dict(epi=QUERY_MAX, ws_short=1), WORKSPACE, b"workspace needs"),
    ("fp32 features", dict(ft=_abi.SAF_F32), UNSUPPORTED, b"SAF_F16 or SAF_BF16"),
    ("no text", dict(text=None), INVALID, b"bad arguments"),
    ("no queries", dict(q=0), INVALID, b"bad arguments"),
    ("negative rows", dict(n=-1), INVALID, b"bad arguments"),
]


@pytest.mark.parametrize("what,change,code,names", EX_REFUSALS, ids=[c[0] for c in EX_REFUSALS])
def test_wide_ex_refuses_on_the_host(what, change, code, names):
    rc, msg = _ex(**change)
    assert rc == code, f"{what}: status {rc}, expected {code}: {msg!r}"
    assert msg.startswith(b"wide scan") and names in msg, f"{what}: the error does not name it: {msg!r}"


def test_wide_ex_row_limit_is_exact():
    """row_offset + n_rows = 2^32 - 1 is the last count the per-query maximum's 32-bit row key holds: that call passes the row
    check (it is refused further on, for the workspace this test withholds); one more row does not."""
    rc, msg = _ex(epi=QUERY_MAX, off=(1 << 32) - 1001, ws=None)
    assert rc == WORKSPACE, (rc, msg)
    rc, msg = _ex(epi=QUERY_MAX, off=(1 << 32) - 1000, ws=None)
    assert rc == UNSUPPORTED and b"below 2^32" in msg, (rc, msg)


def test_wide_ex_workspace_size():
    """two tiles' worth of 16-bit text per 32 columns, in whole 256 bytes, and a 64-bit key per padded column; the heat maps' backgrounds
    take a tile of their own; 0 for sizes that make no sense"""
    l = _lib.lib()
    wb = l.saf_query_wide_ex_workspace_bytes
    assert wb(40, 512, SCORES, 0) == 64 * 512 * 2 + 64 * 8
    assert wb(40, 256, QUERY_MAX, 0) == 64 * 256 * 2 + 64 * 8
    assert wb(36, 512, VS_BG, 4) == 64 * 512 * 2 + 64 * 8      # 4 backgrounds in tile 0, 32 targets in tile 1
    assert wb(37, 512, VS_BG, 4) == 96 * 512 * 2 + 96 * 8      # the 33rd target opens a third tile
    assert wb(0, 512, SCORES, 0) == 0 and wb(40, 0, SCORES, 0) == 0 and wb(40, 512, VS_BG, 41) == 0 and wb(40, 512, VS_BG, -1) == 0
    assert l.saf_query_wide_workspace_bytes(40, 128) == 64 * 128 * 2 and l.saf_query_wide_workspace_bytes(0, 128) == 0


def _first(**change):
    """saf_query_scan_wide (the first kernel: feat_dim 128, 256 or 512, scores only) on a call that is fine except for `change`"""
    l = _lib.lib()
    a = dict(feats=P, ft=_abi.SAF_BF16, n=1000, fs=128, d=128, text=P, q=40, ts=128, scale=1.0, norm=_abi.SAF_NORM_L2, out=P,
             ot=_abi.SAF_F32, os=40, ws=P, ws_short=0)
    a.update(change)
    need = l.saf_query_wide_workspace_bytes(a["q"], a["d"])
    rc = l.saf_query_scan_wide(a["feats"], a["ft"], a["n"], a["fs"], a["d"], a["text"], a["q"], a["ts"], a["scale"], a["norm"], a["out"],
                               a["ot"], a["os"], a["ws"], max(need, 16) - a["ws_short"], None)
    return rc, l.saf_last_error()


FIRST_REFUSALS = [
    ("feat_stride not a multiple of 8", dict(fs=132), INVALID, b"feat_stride a multiple of 8"),
    ("feats off 16 bytes", dict(feats=P + 2), INVALID, b"feats on 16 bytes"),
    ("feat_stride below feat_dim", dict(fs=120), INVALID, b"feat_stride 120 is below feat_dim 128"),
    ("text_stride below feat_dim", dict(ts=127), INVALID, b"text_stride 127 is below feat_dim 128"),
    ("out_stride below n_text", dict(os=39), INVALID, b"out_stride 39 is below n_text 40"),
    ("no out", dict(out=None), INVALID, b"bad arguments"),
    ("no workspace", dict(ws=None), WORKSPACE, b"workspace needs"),
    ("workspace off 16 bytes", dict(ws=P + 8), WORKSPACE, b"workspace needs"),
    ("workspace one byte short", dict(ws_short=1), WORKSPACE, b"workspace needs"),
    ("fp32 features", dict(ft=_abi.SAF_F32), UNSUPPORTED, b"SAF_F16 or SAF_BF16"),
]


@pytest.mark.parametrize("what,change,code,names", FIRST_REFUSALS, ids=[c[0] for c in FIRST_REFUSALS])
def test_wide_first_kernel_refuses_on_the_host(what, change, code, names):
    rc, msg = _first(**change)
    assert rc == code, f"{what}: status {rc}, expected {code}: {msg!r}"
    assert msg.startswith(b"wide scan") and names in msg, f"{what}: the error does not name it: {msg!r}"


def test_wide_first_kernel_no_rows_is_no_work():
    """the call the refusals above are variations of is a good one: with no rows it returns SAF_OK before anything is launched"""
    rc, msg = _first(n=0)
    assert rc == 0, (rc, msg)
