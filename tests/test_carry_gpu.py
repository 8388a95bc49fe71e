"""GPU: a fused volume moved to new bounds on its lattice (``move_grid``; include/saf.h: saf_volume_carry, csrc/saf_carry.hip).

(a), (b): the device pass against its NumPy restatement (tests/carry_reference.py) on random buffers, byte for byte.
(c) - (f): the property the feature exists for -- two boxes of one lattice have bit-identical voxel centres on the indices they
share, and which voxels a frame touches depends on the frame and the centre alone, so a volume fused over box A, moved to box B
and fused further IS, on A n B, the volume that fused all the frames over B, and on B \\ A the volume that fused the later frames
only: compared bit for bit wherever the fusion path itself is bit-reproducible (per-frame pipeline, frame-ordered windows), and at
the project's own bar for the order-free default form (tests/test_sums_form.py: 1e-4 of the row's largest magnitude; an fp16
volume: 3 x 2^-11, README "Tolerance")."""
import ctypes as C

import numpy as np
import pytest
import torch

from spatially_aware_ai_amd import _abi
from spatially_aware_ai_amd import synthetic as syn
from spatially_aware_ai_amd._lib import check, lib
from spatially_aware_ai_amd.clipfusion import _axis_tables

import carry_reference as ref
from test_brick_form import _feat_close

pytestmark = pytest.mark.gpu

# ---- (a) the pass on random buffers -------------------------------------------------------------------------------------------
TORCH_DT = {_abi.SAF_F32: torch.float32, _abi.SAF_BF16: torch.bfloat16, _abi.SAF_F16: torch.float16}
SENTINEL = {"tsdf": -123.25, "tsdf_weight": -77, "weight": -78, "rgb": -5.5, "labels_one_hot": -9, "aux": -1234}
FEAT_SENTINEL = 0x5A  # every byte of a destination feature row


def _bits(t):
    """An integer view: values are compared as the bytes they are (NaN rows included)."""
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()]) if t.is_floating_point() else t


def _random_source(nvox, dim, dt, classes, aux, rng):
    """CPU tensors of a source volume: about half the voxels untouched, and the rows of those are NaN (labels: a poison value)."""
    n = int(np.prod(nvox))
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    weight = torch.from_numpy(rng.integers(0, 3, n).astype(np.int32) * rng.integers(0, 2, n).astype(np.int32))
    v = {"tsdf": torch.randn(n, generator=g), "tsdf_weight": torch.from_numpy(rng.integers(0, 2, n).astype(np.int32) * 5),
         "weight": weight, "rgb": torch.rand(n, 3, generator=g), "clip_feat": torch.randn(n, dim, generator=g).to(TORCH_DT[dt])}
    v["clip_feat"][weight == 0] = float("nan")
    if classes:
        v["labels_one_hot"] = torch.from_numpy(rng.integers(0, 50, (n, classes)).astype(np.int32))
        v["labels_one_hot"][weight == 0] = -(1 << 30)
    if aux:
        v["aux"] = torch.from_numpy(rng.integers(-5, 100, n).astype(np.int32))
    return v


def _sentinel_destination(src, nvox):
    n = int(np.prod(nvox))
    out = {}
    for name, t in src.items():
        if name == "clip_feat":
            out[name] = torch.full((n,) + tuple(t.shape[1:]), FEAT_SENTINEL, dtype=torch.uint8).repeat_interleave(t.element_size(), dim=1) \
                .view(t.dtype)
        else:
            out[name] = torch.full((n,) + tuple(t.shape[1:]), SENTINEL[name], dtype=t.dtype)
    return out


def _to_device(v, misalign=False):
    """The volume's tensors on the device; ``misalign``: the feature buffer starts 4 bytes into a larger allocation."""
    out = {k: t.cuda() for k, t in v.items()}
    if misalign:
        f = v["clip_feat"]
        pad = 4 // f.element_size()
        big = torch.empty(f.numel() + pad, dtype=f.dtype, device="cuda")
        out["clip_feat"] = big[pad:].view(f.shape)
        out["clip_feat"].copy_(f)
        assert out["clip_feat"].data_ptr() % 16 == 4
    return out


def _descriptor(v, nvox, dim, dt):
    p = _abi.ptr
    lab = v.get("labels_one_hot")
    return _abi.SafVolume(nvox[0], nvox[1], nvox[2], dim, 0 if lab is None else int(lab.shape[1]), dt, 0, 0.0, None, None, None,
                          p(v["tsdf"]), p(v["tsdf_weight"]), p(v["weight"]), p(v["rgb"]), p(v["clip_feat"]), p(lab))


def _as_grids(v, nvox):
    """NumPy copies shaped by the grid, floats as their bit patterns."""
    return {k: _bits(t).cpu().numpy().reshape(tuple(nvox) + tuple(t.shape[1:])).copy() for k, t in v.items()}


S, D_ = (9, 7, 13), (12, 5, 20)
PASS_CASES = [
    # src, dst, off, D, dtype, classes, aux, misaligned (0 no, 1 destination, 2 source)
    pytest.param(S, D_, (-2, 1, -5), 512, _abi.SAF_F32, 143, True, 0, id="D512-f32-labels-aux"),
    pytest.param(S, D_, (3, -1, 4), 8, _abi.SAF_F32, 0, False, 0, id="D8-f32"),
    pytest.param(S, D_, (0, 0, 0), 6, _abi.SAF_F32, 143, False, 0, id="D6-f32-24-byte-rows-labels"),
    pytest.param(S, D_, (8, 6, 12), 512, _abi.SAF_BF16, 143, True, 0, id="one-voxel-bf16"),
    pytest.param(S, D_, (2, 4, 10), 512, _abi.SAF_F16, 0, True, 0, id="63-voxels-fp16"),
    pytest.param(S, D_, (5, 3, 9), 512, _abi.SAF_F32, 143, False, 0, id="64-voxels"),
    pytest.param(S, D_, (4, 6, 0), 12, _abi.SAF_F16, 143, True, 0, id="65-voxels-D12-fp16-24-byte-rows"),
    pytest.param(S, D_, (20, 0, 0), 8, _abi.SAF_F32, 143, True, 0, id="disjoint"),
    pytest.param(S, (5, 3, 6), (2, 2, 3), 512, _abi.SAF_BF16, 0, False, 0, id="crop-bf16"),
    pytest.param((5, 3, 6), S, (-2, -2, -3), 8, _abi.SAF_F32, 143, True, 0, id="grow"),
    pytest.param(S, D_, (-2, 1, -5), 512, _abi.SAF_F32, 0, False, 1, id="D512-f32-destination-off-16-bytes"),
    pytest.param(S, D_, (3, -1, 4), 512, _abi.SAF_F16, 143, True, 2, id="D512-fp16-source-off-16-bytes"),
]
N_OVERLAP = {"one-voxel-bf16": 1, "63-voxels-fp16": 63, "64-voxels": 64, "65-voxels-D12-fp16-24-byte-rows": 65, "disjoint": 0}


@pytest.mark.parametrize("s_n,d_n,off,dim,dt,classes,aux,misaligned", PASS_CASES)
def test_pass_equals_its_restatement_and_touches_nothing_else(request, s_n, d_n, off, dim, dt, classes, aux, misaligned):
    rng = np.random.default_rng(abs(hash((s_n, d_n, off, dim, dt))) % (1 << 32))
    src = _random_source(s_n, dim, dt, classes, aux, rng)
    ov = ref.overlap(s_n, d_n, off)
    if ov is not None:  # (a tiny overlap must not be all untouched by chance: its first voxel is touched)
        first = np.ravel_multi_index(tuple(sl.start for sl in ov[1]), s_n)
        src["weight"][first] = 2
        src["clip_feat"][first] = 1.5
        if classes:
            src["labels_one_hot"][first] = 3
    dst = _sentinel_destination(src, d_n)
    want, (rows, tsdf) = ref.carry(_as_grids(src, s_n), _as_grids(dst, d_n), off)
    inside, touched = ref.written_masks(_as_grids(src, s_n), d_n, off)
    case = request.node.callspec.id
    if case in N_OVERLAP:
        assert int(inside.sum()) == N_OVERLAP[case]
    if ov is not None:
        assert rows >= 1 and (inside.sum() < 8 or rows < inside.sum()), "the case does not exercise both kinds of voxel"
    s_dev, d_dev = _to_device(src, misaligned == 2), _to_device(dst, misaligned == 1)
    counts = torch.tensor([5, 7], dtype=torch.int64, device="cuda")
    vs, vd = _descriptor(s_dev, s_n, dim, dt), _descriptor(d_dev, d_n, dim, dt)
    rc = lib().saf_volume_carry(C.byref(vs), C.byref(vd), off[0], off[1], off[2], _abi.ptr(s_dev.get("aux")), _abi.ptr(d_dev.get("aux")),
                                counts.data_ptr(), None)
    check(rc, "saf_volume_carry")
    torch.cuda.synchronize()
    got = _as_grids(d_dev, d_n)
    for name in want:
        assert np.array_equal(got[name], want[name]), f"{name} differs from the restatement"
    # said once more without the restatement's help: outside the overlap, and in the rows of untouched voxels, the sentinel stands
    before = _as_grids(dst, d_n)
    for name in got:
        keep = ~touched if name in ref.ROWS else ~inside
        assert np.array_equal(got[name][keep], before[name][keep]), f"{name} was written where it must not be"
    assert counts.tolist() == [5 + rows, 7 + tsdf], "the counters are added to, exactly"
    # ... and the source is only read
    for name, t in src.items():
        assert torch.equal(_bits(s_dev[name]).cpu(), _bits(t)), f"the source's {name} changed"


# ---- (b) offsets beyond 2^31 elements and 4 GB --------------------------------------------------------------------------------
def test_pass_addresses_rows_beyond_4_gigabytes():
    dim, s_n, d_n = 8192, (64, 64, 65), (64, 64, 66)
    ns, nd = int(np.prod(s_n)), int(np.prod(d_n))
    assert ns * dim > 1 << 31 and ns * dim * 2 > 1 << 32
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(5)
    last = torch.arange(ns - 100, ns, device=dev)
    src = {"tsdf": torch.zeros(ns, device=dev), "tsdf_weight": torch.zeros(ns, dtype=torch.int32, device=dev),
           "weight": torch.zeros(ns, dtype=torch.int32, device=dev), "rgb": torch.zeros(ns, 3, device=dev),
           "clip_feat": torch.empty((ns, dim), dtype=torch.bfloat16, device=dev)}  # (untouched rows: whatever the allocator left)
    src["weight"][last] = 1
    src["clip_feat"][last] = torch.randn((100, dim), generator=g, device=dev).to(torch.bfloat16)
    dst = {"tsdf": torch.zeros(nd, device=dev), "tsdf_weight": torch.zeros(nd, dtype=torch.int32, device=dev),
           "weight": torch.zeros(nd, dtype=torch.int32, device=dev), "rgb": torch.zeros(nd, 3, device=dev),
           "clip_feat": torch.zeros((nd, dim), dtype=torch.bfloat16, device=dev)}
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    vs, vd = _descriptor(src, s_n, dim, _abi.SAF_BF16), _descriptor(dst, d_n, dim, _abi.SAF_BF16)
    check(lib().saf_volume_carry(C.byref(vs), C.byref(vd), 0, 0, 0, None, None, counts.data_ptr(), None), "saf_volume_carry")
    torch.cuda.synchronize()
    x, y, z = last // (s_n[1] * s_n[2]), (last // s_n[2]) % s_n[1], last % s_n[2]
    there = (x * d_n[1] + y) * d_n[2] + z  # the same voxels in the destination's numbering
    assert int(there.min()) * dim * 2 > 1 << 32
    assert torch.equal(_bits(dst["clip_feat"].index_select(0, there)), _bits(src["clip_feat"].index_select(0, last)))
    assert counts.tolist() == [100, 0] and int(dst["weight"].sum()) == 100 and bool((dst["weight"][there] == 1).all())
    untouched = torch.ones(nd, dtype=torch.bool, device=dev)
    untouched[there] = False
    sample = torch.cat((torch.arange(0, nd, 997, device=dev), torch.arange(nd - 300, nd, device=dev)))
    sample = sample[untouched[sample]]
    assert sample.numel() > 400 and int(_bits(dst["clip_feat"].index_select(0, sample)).abs().max()) == 0, "an untouched row was written"


# ---- (c) - (f): modules -------------------------------------------------------------------------------------------------------
W, H = 64, 48
GRID = syn.make_grid((24, 20, 28))
BOX_A = ((0, 0, 0), (24, 20, 28))
BOX_B = ((-3, 2, -4), (30, 24, 33))  # shifted and enlarged: it drops A's y-planes 0 and 1 and adds voxels on five sides
NAMES = ("tsdf", "tsdf_weight", "weight", "rgb", "clip_feat", "labels_one_hot")
_scans = {}


def _scan(dim, n):
    """A scan of the analytic scene with what the backbones would say per frame -- built once per width, never modified."""
    if dim not in _scans or len(_scans[dim]) < n:
        _scans[dim] = syn.SyntheticScan(4100 + dim, n, W, H, dim)
    return _scans[dim]


def _module(scan, box, seem=True, fdt=torch.float32, defer=False, first_frame=0):
    """A module over ``box`` of GRID's lattice whose replay backbones answer from frame ``first_frame`` of the scan on."""
    from spatially_aware_ai_amd import ClipFusion, ClipSeemFusion

    clip, seg = syn.ReplayClip(scan), syn.ReplaySeg(scan)
    clip.calls = seg.calls = first_frame
    off, n = box
    if seem:
        return ClipSeemFusion(GRID.origin, GRID.voxel_size, torch.tensor(n), GRID.trunc, False, 16, 8, clip, seg, feat_dtype=fdt,
                              defer_frames=defer, index_offset=off).cuda()
    return ClipFusion(GRID.origin, GRID.voxel_size, torch.tensor(n), GRID.trunc, False, clip, None, 16, 8, feat_dtype=fdt,
                      defer_frames=defer, index_offset=off).cuda()


def _fuse(fz, frames, seem=True):
    """One batched call."""
    cat = lambda k: torch.cat([f[k] for f in frames]).cuda()
    fz.integrate_features(cat("depth"), cat("rgb"), cat("pose"), cat("K"), cat("feat"),
                          [f["labels"].float().cuda() for f in frames] if seem else None)
    return fz


def _one_by_one(fz, frames):
    """``integrate()`` itself, one frame per call: the backbones are the replay stand-ins."""
    for f in frames:
        fz.integrate(f["depth"].cuda(), f["rgb"].cuda(), f["pose"].cuda(), f["K"].cuda())


def _in_other(box, other):
    """Boolean [nx,ny,nz] (device) over ``box``'s voxels: those that ``other`` holds too."""
    m = []
    for a in range(3):
        i = torch.arange(box[1][a]) + box[0][a]
        m.append((i >= other[0][a]) & (i < other[0][a] + other[1][a]))
    return (m[0][:, None, None] & m[1][None, :, None] & m[2][None, None, :]).cuda()


def _names(seem):
    return NAMES if seem else NAMES[:-1]


def _assert_moved_equals(moved, full, late, seem, feat_tol=None):
    """On A n B every buffer of ``moved`` is ``full``'s, on B \\ A it is ``late``'s; ``feat_tol``: the feature rows are compared
    as the order-free form is, everything else bit for bit all the same."""
    in_a = _in_other(BOX_B, BOX_A).reshape(-1)
    for name in _names(seem):
        got, f, l = getattr(moved, name), getattr(full, name), getattr(late, name)
        want = torch.where(in_a.view(-1, *([1] * (got.dim() - 1))), f, l)
        if name == "clip_feat" and feat_tol is not None:
            _feat_close(got, want, feat_tol, "clip_feat")
        else:
            assert torch.equal(_bits(got), _bits(want)), f"{name}: the moved volume differs from the ones fused over B directly"


def _three_sets(before_a, full, late):
    """Touched voxels in A n B, in B \\ A and in A \\ B -- the test means nothing if one is empty."""
    wa = before_a.view(*BOX_A[1]) > 0
    a_in_b = _in_other(BOX_A, BOX_B)
    b_in_a = _in_other(BOX_B, BOX_A)
    both, lost = int((wa & a_in_b).sum()), int((wa & ~a_in_b).sum())
    gained = int(((late.weight.view(*BOX_B[1]) > 0) & ~b_in_a).sum())
    assert both > 500 and lost > 50 and gained > 100, (both, lost, gained)
    assert int(((full.weight.view(*BOX_B[1]) > 0) & b_in_a).sum()) >= both
    return both, lost, gained


def _scenario(dim, m, n, seem, fdt, monkeypatch=None, form=None):
    """Frames 1..m over A, moved to B, frames m+1..n; and the two modules over B that fuse 1..n and m+1..n directly."""
    if monkeypatch is not None:
        if form is None:
            monkeypatch.delenv("SAF_WIN_FORM", raising=False)
        else:
            monkeypatch.setenv("SAF_WIN_FORM", form)
    scan = _scan(dim, n)
    fr = scan.frames
    moved = _fuse(_module(scan, BOX_A, seem, fdt), fr[:m], seem)
    weight_a, tsdf_weight_a = moved.weight.clone(), moved.tsdf_weight.clone()
    move = moved.move_grid(*BOX_B)
    _fuse(moved, fr[m:n], seem)
    full = _fuse(_module(scan, BOX_B, seem, fdt), fr[:n], seem)
    late = _fuse(_module(scan, BOX_B, seem, fdt), fr[m:n], seem)
    torch.cuda.synchronize()
    both, lost, gained = _three_sets(weight_a, full, late)
    a_in_b = _in_other(BOX_A, BOX_B).reshape(-1)
    assert int(move.rows_carried) == both and int(move.rows_dropped) == lost
    assert int(move.tsdf_carried) == int(((tsdf_weight_a > 0) & a_in_b).sum())
    assert int(move.tsdf_dropped) == int(((tsdf_weight_a > 0) & ~a_in_b).sum()) > 0
    assert move.rows_carried.is_cuda and move.rows_carried.dtype == torch.int64 and move.rows_carried.dim() == 0
    assert (move.old_index_offset, move.old_nvox, move.index_offset, move.nvox) == BOX_A + BOX_B
    assert (move.overlap_in_old, move.overlap_in_new, move.overlap_nvox) == ((0, 2, 0), (3, 0, 4), (24, 18, 28))
    return moved, full, late


@pytest.mark.parametrize("seem", [pytest.param(True, id="ClipSeemFusion"), pytest.param(False, id="ClipFusion")])
def test_moved_then_fused_is_the_volume_fused_over_the_new_box_per_frame_pipeline(seem):
    moved, full, late = _scenario(64, 6, 11, seem, torch.float32)
    assert moved.stats()["window_rows"] == 0
    _assert_moved_equals(moved, full, late, seem)


def test_moved_then_fused_is_the_volume_fused_over_the_new_box_frame_ordered_windows(monkeypatch):
    moved, full, late = _scenario(256, 24, 40, True, torch.float32, monkeypatch, "rows")
    assert moved.stats()["window_rows"] > 0, "the windowed path did not run"
    _assert_moved_equals(moved, full, late, True)


@pytest.mark.parametrize("dim,fdt,tol", [pytest.param(256, torch.float32, 1e-4, id="f32"),
                                         pytest.param(512, torch.float16, 3 * 2.0 ** -11, id="fp16")])
def test_moved_then_fused_in_the_default_form(monkeypatch, dim, fdt, tol):
    """The order-free form folds a window's samples in one update: 24 + 16 frames and 40 frames round differently.  Which voxels
    are touched, the counts, tsdf, rgb and label counts are exact all the same; the feature rows are held to the form's own bar."""
    moved, full, late = _scenario(dim, 24, 40, True, fdt, monkeypatch, None)
    assert moved.stats()["window_rows"] > 0 and moved.stats()["window_form"].startswith("sums")
    _assert_moved_equals(moved, full, late, True, feat_tol=tol)


def test_moved_then_fused_against_the_oracle_on_the_lattice_box(oracle):
    dim, m, n = 64, 6, 11
    moved, _, _ = _scenario(dim, m, n, True, torch.float32)
    fr = _scan(dim, n).frames[:n]
    vol = oracle.OracleVolume(GRID.origin, GRID.voxel_size, torch.tensor(BOX_B[1]), GRID.trunc, dim, 143)
    vol.axes = _axis_tables(GRID.origin, GRID.voxel_size, BOX_B[1], BOX_B[0])
    cat = lambda k: torch.cat([f[k] for f in fr])
    vol.integrate(cat("depth"), cat("rgb"), cat("pose"), cat("K"), cat("feat"), [f["labels"].float() for f in fr], rgb_bilinear=True)
    in_a = _in_other(BOX_B, BOX_A).reshape(-1).cpu()
    for name in ("weight", "tsdf_weight", "labels_one_hot"):
        assert torch.equal(getattr(moved, name).cpu()[in_a], getattr(vol, name)[in_a]), f"{name}: sets differ from the oracle's"
    for name in ("clip_feat", "tsdf", "rgb"):
        np.testing.assert_allclose(getattr(moved, name).cpu()[in_a].numpy(), getattr(vol, name)[in_a].numpy(), rtol=1e-4, atol=1e-6,
                                   err_msg=name)


# ---- (d) behind the queue -----------------------------------------------------------------------------------------------------
def test_move_behind_the_queue_of_one_frame_calls(rows_form):
    """40 one-frame ``integrate()`` calls are queued (the queue hands its session the first 32 on its own, whose window's row
    kernel stays owed, and holds the other 8: nothing has been brought up to date for a reader), ``move_grid`` joins them, 24 more
    follow: bit for bit the direct fusion of 64 frames over B."""
    dim, m, n = 256, 40, 64
    scan = _scan(dim, n)
    fr = scan.frames
    fz = _module(scan, BOX_A, defer=True)
    _one_by_one(fz, fr[:m])
    q = fz.__dict__["_queue"]
    assert fz.pending_frames + q.ring.sess_frames == m and fz.pending_frames > 0 and fz._queue_busy(), "the calls did not go through the queue"
    assert fz.clip.calls == m
    move = fz.move_grid(*BOX_B)
    assert fz.__dict__["_queue"] is q and not fz._queue_busy() and fz.pending_frames == 0
    _one_by_one(fz, fr[m:n])
    assert fz.pending_frames > 0 and fz.clip.calls == n
    full = _fuse(_module(scan, BOX_B), fr[:n])
    late = _fuse(_module(scan, BOX_B), fr[m:n])
    st = fz.stats()
    assert st["frames"] == n and st["window_rows"] > 0
    _assert_moved_equals(fz, full, late, True)
    assert int(move.rows_carried) > 0 and int(move.rows_dropped) > 0


# ---- (e) a source whose deferred clear is still owed --------------------------------------------------------------------------
def test_move_of_a_volume_whose_rows_are_still_stale(rows_form):
    dim = 256
    scan = _scan(dim, 64)
    fr = scan.frames
    fz = _fuse(_module(scan, BOX_A), fr[:24])
    assert float(fz.clip_feat.abs().sum()) > 0
    fz._buffers["clip_feat"].fill_(float("nan"))  # whatever the first scan left must never be seen again
    fz.reset()
    _fuse(fz, fr[24:48])  # (24 frames: the windowed path, which never reads a weight-0 row -- the clear stays owed)
    assert fz._feat_stale and bool(torch.isnan(fz._buffers["clip_feat"]).any())
    fz.move_grid(*BOX_B)
    fresh = _fuse(_module(scan, BOX_B), fr[24:48])
    in_a = _in_other(BOX_B, BOX_A).reshape(-1)
    w = fz.weight
    assert int((w > 0).sum()) > 500
    assert int(_bits(fz.clip_feat)[w == 0].abs().max()) == 0, "a row of an untouched voxel does not read as zero"
    for name in NAMES:
        got, want = getattr(fz, name), getattr(fresh, name)
        assert torch.equal(_bits(got)[in_a], _bits(want)[in_a]), f"{name} differs from a fresh module's on the shared voxels"
        assert int(_bits(got)[~in_a].abs().max()) == 0, f"{name}: the voxels the new box adds are not empty"


# ---- (f) the module afterwards ------------------------------------------------------------------------------------------------
def test_module_state_after_the_move():
    dim, m, n = 64, 6, 11
    scan = _scan(dim, n)
    fr = scan.frames
    fz = _fuse(_module(scan, BOX_A), fr[:m])
    n_a = int(np.prod(BOX_A[1]))
    fz.voxel_obj_idx = (torch.arange(n_a, dtype=torch.int32, device="cuda") % 1000 - 2).view(*BOX_A[1])
    fz.objects_segmentation_color = torch.rand(n_a, 3, device="cuda")
    stats_ptr, clip, seg = fz._buffers["fuse_stats"].data_ptr(), fz.clip, fz.segmentation_model
    fz.move_grid(*BOX_B)
    twin = _module(scan, BOX_B)
    assert [int(v) for v in fz.nvox] == [int(v) for v in twin.nvox] and fz.index_offset == twin.index_offset == BOX_B[0]
    for name in ("axis_x", "axis_y", "axis_z", "xyz_world"):
        assert torch.equal(_bits(fz._buffers[name]), _bits(twin._buffers[name])), name
    assert fz._buffers["fuse_stats"].data_ptr() == stats_ptr and fz.clip is clip and fz.segmentation_model is seg
    assert fz._workspace is None and not hasattr(fz, "objects_segmentation_color")
    # voxel_obj_idx: carried, -1 where the new box adds voxels
    src = {"weight": np.ones(BOX_A[1], np.int32), "tsdf_weight": np.ones(BOX_A[1], np.int32), "tsdf": np.zeros(BOX_A[1], np.float32),
           "rgb": np.zeros(BOX_A[1] + (3,), np.float32), "aux": (np.arange(n_a, dtype=np.int32) % 1000 - 2).reshape(BOX_A[1])}
    dst = {k: np.full(BOX_B[1] + v.shape[3:], -1, v.dtype) for k, v in src.items()}
    off = tuple(b - a for a, b in zip(BOX_A[0], BOX_B[0]))
    want = ref.carry(src, dst, off)[0]["aux"]
    assert tuple(fz.voxel_obj_idx.shape) == BOX_B[1] and np.array_equal(fz.voxel_obj_idx.cpu().numpy(), want)
    assert int((fz.voxel_obj_idx == -1).sum()) >= int((~_in_other(BOX_B, BOX_A)).sum()) > 0
    # the moved module works: labels, a view, statistics, frames in and out again
    lab = fz.label_index()
    assert lab.shape == (int(np.prod(BOX_B[1])),) and int((lab >= 0).sum()) > 0 and not bool((lab[fz.weight == 0] >= 0).any())
    out = fz.render(fr[0]["pose"][0].cuda(), fr[0]["K"][0].cuda(), H, W)
    assert int(out.hit.sum()) > 0 and int(out.voxel.max()) < lab.numel() and int(out.label.max()) >= 0
    snap = {name: getattr(fz, name).clone() for name in NAMES}
    _fuse(fz, fr[m:n])
    assert fz._workspace is not None, "the workspace was not sized again"
    assert fz.stats()["frames"] == n
    cat = lambda k: torch.cat([f[k] for f in fr[m:n]]).cuda()
    fz.deintegrate_features(cat("depth"), cat("rgb"), cat("pose"), cat("K"), cat("feat"), [f["labels"].float().cuda() for f in fr[m:n]],
                            strict=True)
    for name in ("weight", "tsdf_weight", "labels_one_hot"):
        assert torch.equal(getattr(fz, name), snap[name]), f"{name} after frames went in and out again"
    assert bool(torch.isfinite(fz.clip_feat).all()) and bool(torch.isfinite(fz.tsdf).all())


def test_fp16_module_moves_and_the_wide_scan_still_reads_its_rows_in_place():
    from spatially_aware_ai_amd.distributed import shard_features_16

    dim = 512
    scan = _scan(dim, 40)
    fz = _fuse(_module(scan, BOX_A, fdt=torch.float16), scan.frames[:24])
    before = shard_features_16(fz, 0, 100)
    assert before.data_ptr() == fz.clip_feat.data_ptr()
    fz.move_grid(*BOX_B)
    assert fz.__dict__["_shard16"] is None
    rows = shard_features_16(fz, 50, 200)
    assert rows.dtype == torch.float16 and rows.data_ptr() == fz.clip_feat[50:250].data_ptr(), "not a view of the moved volume's rows"
    assert fz.clip_feat.shape == (int(np.prod(BOX_B[1])), dim) and bool(torch.isfinite(fz.clip_feat.float()).all())
