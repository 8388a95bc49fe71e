"""The device passes of the frame-sharded merge's packed route (csrc/saf_merge.hip; SURVEY section 8e, new capability):
`saf_merge_scan_touched` (positions of the touched rows + the split sizes), `saf_merge_pack_rows` (touched rows -> the send
buffer), `saf_merge_add_packed` (the received contributions added in rank order, in place) against their torch statements
(tests/frame_pass_reference.py: merge_positions, merge_expected) -- bit for bit: the sums are left-to-right in rank order on both
sides.  Every buffer a pass writes has 64 guard elements before and after it, and `dst` is compared whole: rows outside
[first, first + n_rows) and untouched rows inside it stay as they were.  The collectives around them are tested under gloo at
world 2 / 4 / 8 (tests/test_distributed_cpu.py) and under RCCL at world 1 (tests/test_nccl_world1.py)."""
import ctypes as C

import pytest
import torch

import frame_pass_reference as R

pytestmark = pytest.mark.gpu

G = R.GUARD
DEV = torch.device("cuda", 0)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(rows, tail, dt, fill, off=0):
    """[rows, *tail] of `dt` inside a flat buffer: G guard elements before and after, `off` more elements (4 bytes each) in front
    -- off = 1 puts the view 4 bytes off the allocation's alignment.  (whole buffer, view)"""
    n = rows
    for d in tail:
        n *= d
    buf = torch.full((G + off + n + G,), fill, dtype=dt, device=DEV)
    return buf, buf[G + off:G + off + n].view((rows,) + tuple(tail))


def _ptr(buf, view):
    """The view's address (an empty view has none of its own: its place between the guards)."""
    return buf.data_ptr() + view.storage_offset() * buf.element_size()


def _guards_intact(buf, view, fill):
    lo = view.storage_offset()
    return bool((buf[:lo] == fill).all()) and bool((buf[lo + view.numel():] == fill).all())


def _weights(n, share, g, negatives=False):
    w = (torch.rand(n, generator=g, device=DEV) < share).int() * torch.randint(1, 9, (n,), generator=g, device=DEV, dtype=torch.int32)
    if negatives:  # a third of the untouched rows get a negative weight: not touched either
        w = torch.where((w == 0) & (torch.rand(n, generator=g, device=DEV) < 0.33), torch.full_like(w, -3), w)
    return w


def _scan(w, bounds=None):
    """saf_merge_scan_touched; checks pos (and the offsets at `bounds`) against the statement, returns pos."""
    from spatially_aware_ai_amd._lib import check, lib

    L, n = lib(), w.numel()
    nb = 0 if bounds is None else len(bounds)
    pos_buf, pos = _guarded(n + 1, (), torch.int32, -5)
    ws = torch.empty(max(256, L.saf_merge_scan_workspace_bytes(n, nb)), dtype=torch.uint8, device=DEV)  # (more than asked for is fine)
    bd = host = None
    if nb:
        bd = torch.tensor(bounds, dtype=torch.int64, device=DEV)
        host = torch.full((nb,), -5, dtype=torch.int32).pin_memory()
    check(L.saf_merge_scan_touched(w.data_ptr(), n, pos.data_ptr(), None if bd is None else bd.data_ptr(), nb,
                                   None if host is None else host.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "scan")
    torch.cuda.synchronize()
    want = R.merge_positions(w)
    assert torch.equal(pos, want) and _guards_intact(pos_buf, pos, -5)
    if nb:
        assert host.tolist() == want[bd].tolist()
    return pos


def _pack_and_add(t, w, pos, pack_range, add_range, world, g, off=(0, 0, 0, 0)):
    """Pack the touched rows of pack_range, add `world` contributions into the touched rows of add_range; `off` = element
    offsets of (src, send, dst, recv) into their buffers."""
    from spatially_aware_ai_amd._lib import check, lib

    L, dt, tail = lib(), t.dtype, tuple(t.shape[1:])
    row_bytes = 4
    for d in tail:
        row_bytes *= d
    n = t.shape[0]
    src_buf, src = _guarded(n, tail, dt, 0, off[0])
    src.copy_(t)
    # pack
    first, rows = pack_range
    want_send = R.merge_expected(t, w, first, rows)
    send_buf, send = _guarded(len(want_send), tail, dt, 7, off[1])
    check(L.saf_merge_pack_rows(src.data_ptr(), row_bytes, w.data_ptr(), pos.data_ptr(), first, rows, _ptr(send_buf, send), _stream()), "pack")
    assert torch.equal(send, want_send), "packed rows"
    assert _guards_intact(send_buf, send, 7), "pack wrote outside the send buffer"
    assert torch.equal(src, t)
    # add
    first, rows = add_range
    mine = int(pos[first + rows]) - int(pos[first])
    recv_buf, recv = _guarded(world * mine, tail, dt, 0, off[3])
    recv.copy_((torch.randn((world * mine,) + tail, generator=g, device=DEV) * 100).to(dt))
    dst_buf, dst = _guarded(n, tail, dt, 7, off[2])
    dst.copy_(t)
    check(L.saf_merge_add_packed(dst.data_ptr(), row_bytes, 1 if dt.is_floating_point else 0, w.data_ptr(), pos.data_ptr(), first, rows,
                                 _ptr(recv_buf, recv), mine, world, _stream()), "add")
    assert torch.equal(dst, R.merge_expected(t, w, first, rows, recv, world)), ("sum in rank order", tail, dt)
    assert _guards_intact(dst_buf, dst, 7), "add wrote outside dst"
    return mine


def _rows(shape, dt, g):
    return (torch.randn(shape, generator=g, device=DEV) * 100).to(dt)


@pytest.mark.parametrize("n,share,world", [(5000, 0.2, 4), (70001, 0.03, 8), (4096, 1.0, 2), (300, 0.0, 5)])
def test_scan_pack_add_against_torch(n, share, world):
    g = torch.Generator(device=DEV).manual_seed(n)
    w = _weights(n, share, g)
    c = n // world
    pos = _scan(w, [k * c for k in range(world + 1)])
    for shape, dt in (((n, 512), torch.float32), ((n, 3), torch.float32), ((n, 143), torch.int32), ((n,), torch.float32)):
        # pack: the rows of parts 1 .. world - 1 (a range that does not start at row 0); add: this "rank" owns the last part
        mine = _pack_and_add(_rows(shape, dt, g), w, pos, (c, (world - 1) * c), ((world - 1) * c, c), world, g)
        assert (mine == 0) == (share == 0.0)  # (no touched rows: add returns OK and leaves dst alone)


@pytest.mark.parametrize("row_elems", [4, 1], ids=["row16B", "row4B"])
def test_grid_stride_loop_runs_more_than_once(row_elems):
    """grid_1d(n_rows, 16) caps the grid at CUs * 16 workgroups of 256 rows: above CUs * 16 * 256 rows a wave's loop
    `r0 += n_waves * 64` iterates again (production, 256^3 rows: 16 times).  Here twice, and a third ragged time."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = cus * 16 * 256 * 2 + 77
    assert n > cus * 16 * 256
    g = torch.Generator(device=DEV).manual_seed(row_elems)
    w = _weights(n, 0.3, g)
    pos = _scan(w, [0, n // 3, n])
    t = _rows((n, row_elems) if row_elems > 1 else (n,), torch.float32, g)
    _pack_and_add(t, w, pos, (0, n), (0, n), 3, g)


@pytest.mark.parametrize("world", [1, 3, 6, 7, 9])
def test_world_sizes_and_the_unrolled_sum_remainders(world):
    """The vector path adds four contributions per step after the first: world 1 (no addition), 3 (remainder only), 6 and 7
    (one step + remainders 1 and 2), 9 (two steps, no remainder)."""
    n = 5000
    g = torch.Generator(device=DEV).manual_seed(world)
    w = _weights(n, 0.2, g)
    pos = _scan(w)
    for shape, dt in (((n, 512), torch.float32), ((n, 143), torch.int32)):
        assert _pack_and_add(_rows(shape, dt, g), w, pos, (100, n - 300), (1000, 3000), world, g) > 0


@pytest.mark.parametrize("which", ["src", "send", "dst", "recv"])
@pytest.mark.parametrize("dt", [torch.float32, torch.int32], ids=["f32", "i32"])
def test_wide_rows_on_a_misaligned_pointer(which, dt):
    """row_bytes % 16 == 0 with one of the four buffers a view 4 bytes into its allocation: the 16-byte path must not be taken
    (vec == 0 with wide rows)."""
    n = 5000
    g = torch.Generator(device=DEV).manual_seed(11)
    w = _weights(n, 0.2, g)
    pos = _scan(w)
    off = tuple(int(k == which) for k in ("src", "send", "dst", "recv"))
    for world in (3, 6):
        assert _pack_and_add(_rows((n, 16), dt, g), w, pos, (100, n - 300), (1000, 3000), world, g, off) > 0
    # 2 KiB rows: the 4-byte loop takes eight steps per lane
    assert _pack_and_add(_rows((n, 512), dt, g), w, pos, (100, n - 300), (1000, 3000), 6, g, off) > 0


@pytest.mark.parametrize("share", [0.5, 1.0])
def test_a_short_range_off_a_multiple_of_64(share):
    n = 300
    g = torch.Generator(device=DEV).manual_seed(37)
    w = _weights(n, share, g)
    pos = _scan(w)
    for shape, dt in (((n, 512), torch.float32), ((n, 143), torch.int32), ((n,), torch.float32)):
        assert _pack_and_add(_rows(shape, dt, g), w, pos, (37, 50), (37, 50), 3, g) > 0
        assert _pack_and_add(_rows(shape, dt, g), w, pos, (37, 0), (37, 0), 3, g) == 0  # an empty range: OK, nothing moves


def test_non_positive_weights_are_not_touched():
    """weight < 0 counts as not touched, in the scan and in both passes: with negatives among touched rows, and with nothing
    touched at all (pack writes nothing, add has mine == 0 and leaves dst alone)."""
    n = 5000
    g = torch.Generator(device=DEV).manual_seed(5)
    mixed = _weights(n, 0.2, g, negatives=True)
    none = torch.where(torch.rand(n, generator=g, device=DEV) < 0.5, torch.full((n,), -2, dtype=torch.int32, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV))
    assert int((mixed < 0).sum()) > 500 and int((mixed > 0).sum()) > 500 and int((none < 0).sum()) > 500
    for w in (mixed, none):
        pos = _scan(w, [0, 1234, n])
        for shape, dt in (((n, 512), torch.float32), ((n, 143), torch.int32)):
            mine = _pack_and_add(_rows(shape, dt, g), w, pos, (100, n - 300), (1000, 3000), 3, g)
            assert (mine == 0) == (w is none)


def test_scan_edges():
    """One row (touched, untouched, negative) and a scan without bounds."""
    for v in (3, 0, -1):
        w = torch.tensor([v], dtype=torch.int32, device=DEV)
        assert _scan(w).tolist() == [0, int(v > 0)]
        assert _scan(w, [0, 1, 1]).tolist() == [0, int(v > 0)]
    g = torch.Generator(device=DEV).manual_seed(1)
    _scan(_weights(70001, 0.5, g, negatives=True))


def test_refusals():
    from spatially_aware_ai_amd import _abi
    from spatially_aware_ai_amd._lib import lib

    L, n = lib(), 256
    w = torch.ones(n, dtype=torch.int32, device=DEV)
    pos = _scan(w)
    t = torch.zeros((n, 6), device=DEV)
    send_buf, send = _guarded(n, (6,), torch.float32, 7)
    p = lambda x: x.data_ptr()
    assert L.saf_merge_pack_rows(p(t), 6, p(w), p(pos), 0, n, p(send), _stream()) == _abi.SAF_E_INVALID      # row_bytes % 4 != 0
    assert L.saf_merge_add_packed(p(send), 6, 1, p(w), p(pos), 0, n, p(t), n, 1, _stream()) == _abi.SAF_E_INVALID
    assert L.saf_merge_add_packed(p(send), 24, 1, p(w), p(pos), 0, n, p(t), n, 0, _stream()) == _abi.SAF_E_INVALID  # world < 1
    assert L.saf_merge_add_packed(p(send), 24, 1, p(w), p(pos), 0, n, p(t), n, -2, _stream()) == _abi.SAF_E_INVALID
    need = L.saf_merge_scan_workspace_bytes(n, 2)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    pos2 = torch.full((n + 1,), -5, dtype=torch.int32, device=DEV)
    bd = torch.tensor([0, n], dtype=torch.int64, device=DEV)
    host = torch.full((2,), -5, dtype=torch.int32).pin_memory()
    assert need > 0
    assert L.saf_merge_scan_touched(p(w), n, p(pos2), p(bd), 2, p(host), p(ws), need - 1, _stream()) == _abi.SAF_E_WORKSPACE
    torch.cuda.synchronize()
    assert bool((send_buf == 7).all()) and bool((pos2 == -5).all()) and host.tolist() == [-5, -5], "a refused call wrote nothing"
    assert L.saf_merge_scan_touched(p(w), n, p(pos2), p(bd), 2, p(host), p(ws), need, _stream()) == _abi.SAF_OK
    torch.cuda.synchronize()
    assert host.tolist() == [0, n]
