"""CPU: absorbing a second fused volume of the same lattice (``absorb``, ``join_scenes``; include/saf.h: saf_volume_absorb) as far
as it can be checked without a GPU -- the NumPy restatement (tests/absorb_reference.py) on itself, the refusals the library decides
on the host, ``absorb()``'s own refusals, and the box ``reconstruct_scene(lattice_of=...)`` chooses."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from spatially_aware_ai_amd import _abi, _lib
from spatially_aware_ai_amd import synthetic as syn
from spatially_aware_ai_amd._lib import SafError
from spatially_aware_ai_amd.clipfusion import lattice_box

import absorb_reference as ref
from host_stubs import P, fake_volume

FAR = 1 << 40  # the destination's stand-in pointers: far from the source's, so that no byte range intersects
GRID = syn.make_grid((12, 10, 14))


# ---- the restatement on itself ------------------------------------------------------------------------------------------------
def _volume(n, dim, rng, classes=0, weights=None):
    w = rng.integers(0, 2, n).astype(np.int32) * rng.integers(1, 301, n).astype(np.int32) if weights is None else weights
    tw = rng.integers(0, 2, n).astype(np.int32) * rng.integers(1, 301, n).astype(np.int32) if weights is None else weights
    v = {"tsdf": rng.standard_normal(n).astype(np.float32), "tsdf_weight": tw.astype(np.int32), "weight": w.astype(np.int32),
         "rgb": rng.random(n + (3,)).astype(np.float32), "clip_feat": rng.standard_normal(n + (dim,)).astype(np.float32)}
    if classes:
        v["labels_one_hot"] = rng.integers(0, 50, n + (classes,)).astype(np.int32)
    return v


def _copy(v):
    return {k: a.copy() for k, a in v.items()}


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def test_a_one_sample_source_is_one_running_mean_step_bit_for_bit():
    """saf_fuse_frames' update (include/saf.h: SAF_RUNNING_MEAN) is x <- s * (1 / w') + x * (w * (1 / w')), w' = w + 1; absorbing
    a volume that holds ONE sample s at weight 1 must be exactly that step, for every count the volume may have."""
    rng = np.random.default_rng(1)
    n, dim = (300, 1, 1), 7
    w = np.arange(1, 301, dtype=np.int32).reshape(n)
    dst = _volume(n, dim, rng, classes=5, weights=w)
    src = _volume(n, dim, rng, classes=5, weights=np.ones(n, np.int32))
    out, counts = ref.absorb(src, _copy(dst), (0, 0, 0))
    assert counts == (300, 0, 300, 0)
    a = np.float32(1.0) / (w + 1).astype(np.float32)
    b = w.astype(np.float32) * a
    for name, ca, cb in (("tsdf", a, b), ("rgb", a[..., None], b[..., None]), ("clip_feat", a[..., None], b[..., None])):
        step = (src[name] * ca).astype(np.float32) + (dst[name] * cb).astype(np.float32)
        assert step.dtype == np.float32 and np.array_equal(_bits(out[name]), _bits(step)), name
    assert np.array_equal(out["weight"], w + 1) and np.array_equal(out["tsdf_weight"], w + 1)
    assert np.array_equal(out["labels_one_hot"], dst["labels_one_hot"] + src["labels_one_hot"])


@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
def test_restatement_writes_what_it_should_and_nothing_else(kind):
    rng = np.random.default_rng(2)
    s_n, d_n, off, dim = (5, 4, 6), (7, 3, 6), (-1, 2, 3), 3
    src, dst = _volume(s_n, dim, rng, classes=4), _volume(d_n, dim, rng, classes=4)
    # rows that must never be read: NaN in the source where ws == 0, NaN in the destination where wd == 0
    src["clip_feat"][src["weight"] == 0] = np.nan
    dst["clip_feat"][dst["weight"] == 0] = np.nan
    src["tsdf"][src["tsdf_weight"] == 0] = np.nan
    dst["tsdf"][dst["tsdf_weight"] == 0] = np.nan
    if kind != "f32":
        for v in (src, dst):
            v["clip_feat"] = ref.narrow(v["clip_feat"], kind)
    before = _copy(dst)
    m = ref.written_masks(src, before, off)
    out, counts = ref.absorb(src, dst, off, kind)
    assert m["inside"].sum() == 5 * 2 * 3
    assert counts == (m["blend"].sum(), m["copy"].sum(), m["t_blend"].sum(), m["t_copy"].sum()) and min(counts) > 0
    assert (~m["inside"]).sum() > 0 and (m["inside"] & ~m["copy"] & ~m["blend"]).sum() > 0
    rows, tsdf = m["copy"] | m["blend"], m["t_copy"] | m["t_blend"]
    for name in out:
        keep = ~(tsdf if name in ("tsdf", "tsdf_weight") else rows)
        assert np.array_equal(_bits(out[name])[keep], _bits(before[name])[keep]), f"{name} changed outside the overlap or at ws == 0"
    # what was written is finite: no poisoned row reached the output ...
    assert np.isfinite(ref.widen(out["clip_feat"], kind)[rows]).all() and np.isfinite(out["tsdf"][tsdf]).all()
    # ... a copy is the source's bytes, a blend has the summed count
    for x, y, z in zip(*np.nonzero(m["inside"])):
        sx, sy, sz = x + off[0], y + off[1], z + off[2]
        if m["copy"][x, y, z]:
            assert np.array_equal(_bits(out["clip_feat"][x, y, z]), _bits(src["clip_feat"][sx, sy, sz]))
            assert out["weight"][x, y, z] == src["weight"][sx, sy, sz]
            assert np.array_equal(out["labels_one_hot"][x, y, z], src["labels_one_hot"][sx, sy, sz])
        if m["blend"][x, y, z]:
            assert out["weight"][x, y, z] == src["weight"][sx, sy, sz] + before["weight"][x, y, z]
            lo = np.minimum(ref.widen(src["clip_feat"][sx, sy, sz], kind), ref.widen(before["clip_feat"][x, y, z], kind))
            hi = np.maximum(ref.widen(src["clip_feat"][sx, sy, sz], kind), ref.widen(before["clip_feat"][x, y, z], kind))
            got = ref.widen(out["clip_feat"][x, y, z], kind)
            slack = 2.0 ** -7 * np.maximum(np.abs(lo), np.abs(hi))  # (one bf16 rounding: 2^-9 relative)
            assert ((got >= lo - slack) & (got <= hi + slack)).all(), "a weighted mean lies between its two values"
        if m["t_blend"][x, y, z]:
            assert out["tsdf_weight"][x, y, z] == src["tsdf_weight"][sx, sy, sz] + before["tsdf_weight"][x, y, z]
    assert ref.absorb(src, dst, (9, 0, 0), kind)[1] == (0, 0, 0, 0)


def test_restatement_pins_the_int_to_float_rounding():
    """2^24 + 1 + 1 is representable, 2^24 + 1 is not: (float)wd rounds to even, and the two coefficients no longer sum to 1."""
    one = lambda val, dt: np.full((1, 1, 1), val, dt)
    mk = lambda w, x: {"tsdf": one(x, np.float32), "tsdf_weight": one(w, np.int32), "weight": one(w, np.int32),
                       "rgb": np.full((1, 1, 1, 3), x, np.float32), "clip_feat": np.full((1, 1, 1, 2), x, np.float32)}
    out, _ = ref.absorb(mk(1, 3.0), mk((1 << 24) + 1, 5.0), (0, 0, 0))
    r = np.float32(1.0) / np.float32((1 << 24) + 2)
    want = np.float32(np.float32(3.0) * (np.float32(1.0) * r)) + np.float32(np.float32(5.0) * (np.float32(1 << 24) * r))
    assert out["weight"][0, 0, 0] == (1 << 24) + 2 and out["clip_feat"][0, 0, 0, 0] == want == out["tsdf"][0, 0, 0]


# ---- the entry point's refusals, decided before anything is launched ----------------------------------------------------------
def _pair(n_src=8, n_dst=8, dim=8, dtype=_abi.SAF_F32, classes=0):
    src = fake_volume(n_src, dim, dtype, n_classes=classes, labels_one_hot=P if classes else None)
    dst = fake_volume(n_dst, dim, dtype, n_classes=classes)
    for f in ("tsdf", "tsdf_weight", "weight", "rgb", "clip_feat") + (("labels_one_hot",) if classes else ()):
        setattr(dst, f, FAR)
    return src, dst


def _absorb(src, dst, off=(100, 0, 0), counts=None):
    """(status, message).  The default offset leaves no overlap: a call that passes the checks returns 0 with nothing launched."""
    l = _lib.lib()
    rc = l.saf_volume_absorb(None if src is None else ctypes.byref(src), None if dst is None else ctypes.byref(dst), off[0], off[1],
                             off[2], counts, None)
    return rc, l.saf_last_error().decode()


def test_absorb_accepts_a_well_formed_pair_and_an_empty_overlap_is_ok():
    for off in ((100, 0, 0), (0, -8, 0), (0, 0, 8), (2 ** 31 - 1, 0, 0), (-2 ** 31, 0, 0)):
        assert _absorb(*_pair(), off=off)[0] == 0
    assert _absorb(*_pair(classes=143))[0] == 0
    assert _absorb(*_pair(dim=12, dtype=_abi.SAF_F16))[0] == 0
    assert _absorb(*_pair(dim=512, dtype=_abi.SAF_BF16), counts=P)[0] == 0


def test_absorb_refuses_nulls_and_bad_sizes():
    src, dst = _pair()
    assert _absorb(None, dst)[0] == _abi.SAF_E_INVALID and _absorb(src, None)[0] == _abi.SAF_E_INVALID
    for which in (0, 1):
        for f in ("tsdf", "tsdf_weight", "weight", "rgb", "clip_feat"):
            pair = _pair()
            setattr(pair[which], f, None)
            rc, msg = _absorb(*pair)
            assert rc == _abi.SAF_E_INVALID and "NULL" in msg, (which, f)
        for f in ("nx", "ny", "nz"):
            for bad in (0, -3):
                pair = _pair()
                setattr(pair[which], f, bad)
                assert _absorb(*pair)[0] == _abi.SAF_E_INVALID, (which, f, bad)
        pair = _pair(classes=143)
        pair[which].labels_one_hot = None
        assert _absorb(*pair)[0] == _abi.SAF_E_INVALID
        pair = _pair()
        pair[which].nx, pair[which].ny, pair[which].nz = 2048, 1024, 1024  # 2^31 voxels
        rc, msg = _absorb(*pair)
        assert rc == _abi.SAF_E_INVALID and "2^31" in msg
        pair = _pair()
        pair[which].feat_dtype = 7
        assert _absorb(*pair)[0] == _abi.SAF_E_INVALID
    assert _absorb(*_pair(dim=0))[0] == _abi.SAF_E_INVALID


def test_absorb_refuses_volumes_that_differ():
    for change in (dict(feat_dim=16), dict(feat_dtype=_abi.SAF_BF16), dict(n_classes=143, labels_one_hot=FAR)):
        src, dst = _pair()
        for k, v in change.items():
            setattr(dst, k, v)
        rc, msg = _absorb(src, dst)
        assert rc == _abi.SAF_E_INVALID and "differ" in msg, change


def test_absorb_refuses_a_destination_that_shares_bytes_with_its_source():
    n, dim = 8, 8
    sizes = {"tsdf": 4, "tsdf_weight": 4, "weight": 4, "rgb": 12, "clip_feat": 4 * dim, "labels_one_hot": 4 * 143}
    for f, per_voxel in sizes.items():
        span = n ** 3 * per_voxel
        for delta, aliased in ((0, True), (span - 4, True), (-(span - 4), True), (span, False), (-span, False)):
            src, dst = _pair(classes=143)
            setattr(src, f, FAR // 2)
            setattr(dst, f, FAR // 2 + delta)
            rc, msg = _absorb(src, dst)
            assert (rc == _abi.SAF_E_INVALID and "overlaps its source" in msg) if aliased else rc == 0, (f, delta)
    src = fake_volume(8, 8)
    assert _absorb(src, src, off=(0, 0, 0))[0] == _abi.SAF_E_INVALID, "the whole volume on itself"


def test_absorb_refuses_rows_that_are_not_aligned_to_their_element():
    src, dst = _pair()
    dst.clip_feat = FAR + 2
    rc, msg = _absorb(src, dst)
    assert rc == _abi.SAF_E_INVALID and "aligned" in msg
    src, dst = _pair(dtype=_abi.SAF_F16)
    dst.clip_feat = FAR + 2  # (a 16-bit row may start on any even address)
    assert _absorb(src, dst)[0] == 0


def test_absorb_takes_running_means_only():
    for which in (0, 1):
        pair = _pair()
        pair[which].accum_mode = _abi.SAF_SUM
        rc, msg = _absorb(*pair)
        assert rc == _abi.SAF_E_UNSUPPORTED and "running means" in msg, which
        assert _absorb(*pair, off=(0, 0, 0))[0] == _abi.SAF_E_UNSUPPORTED, "refused on the host, whatever the overlap"


# ---- absorb()'s own refusals ----------------------------------------------------------------------------------------------------
def _cpu_module(nvox=(12, 10, 14), index_offset=(0, 0, 0), x_planes=None, dim=8, seem=False, origin=None, voxel_size=None,
                trunc=None, fdt=torch.float32):
    from spatially_aware_ai_amd import ClipFusion, ClipSeemFusion
    from test_gpu_parity import FakeClip, FakeSeg

    origin = GRID.origin if origin is None else origin
    voxel_size = GRID.voxel_size if voxel_size is None else voxel_size
    trunc = GRID.trunc if trunc is None else trunc
    if seem:
        return ClipSeemFusion(origin, voxel_size, torch.tensor(nvox), trunc, False, 10, 10, FakeClip(dim), FakeSeg(),
                              keep_xyz_world=False, feat_dtype=fdt, index_offset=index_offset, x_planes=x_planes)
    return ClipFusion(origin, voxel_size, torch.tensor(nvox), trunc, False, FakeClip(dim), None, 10, 10, keep_xyz_world=False,
                      feat_dtype=fdt, index_offset=index_offset, x_planes=x_planes)


def _marked(**kw):
    """A host module whose buffers hold a pattern, and a copy of them."""
    fz = _cpu_module(**kw)
    for i, (name, t) in enumerate(fz._buffers.items()):
        if name in ("tsdf", "rgb", "clip_feat", "weight", "tsdf_weight", "labels_one_hot"):
            t.fill_(i + 1)
    return fz, {k: t.clone() for k, t in fz._buffers.items()}


def _assert_untouched(fz, snap, box=((0, 0, 0), (12, 10, 14))):
    assert (fz.index_offset, tuple(int(v) for v in fz.nvox)) == box
    assert set(fz._buffers) == set(snap)
    for name, t in snap.items():
        assert torch.equal(fz._buffers[name], t), name


def _refused(a, b, match, **kw):
    (fa, sa), (fb, sb) = a, b
    with pytest.raises(SafError, match=match):
        fa.absorb(fb, **kw)
    _assert_untouched(fa, sa, (fa.index_offset, tuple(int(v) for v in fa.nvox)))
    _assert_untouched(fb, sb, (fb.index_offset, tuple(int(v) for v in fb.nvox)))


def test_absorb_refuses_itself_slabs_stripes_and_poisoned_modules_and_leaves_both_alone():
    a = _marked()
    with pytest.raises(SafError, match="itself"):
        a[0].absorb(a[0])
    _assert_untouched(*a)
    with pytest.raises(SafError, match="fusion module"):
        a[0].absorb(SimpleNamespace())
    planes = dict(nvox=(8, 10, 14), x_planes=[0, 1, 2, 3, 8, 9, 10, 11])
    _refused(_marked(**planes), _marked(), "x_planes")
    _refused(_marked(), _marked(**planes), "x_planes")
    for which in (0, 1):
        pair = [_marked(), _marked(index_offset=(-3, 2, 1))]
        pair[which][0]._shard_stripes = [(0, 100)]
        _refused(*pair, "stripes")
        pair = [_marked(), _marked(index_offset=(-3, 2, 1))]
        pair[which][0].__dict__["_poisoned"] = "a flush failed"
        _refused(*pair, "a flush failed")


def test_absorb_refuses_another_device_lattice_or_layout_and_leaves_both_alone():
    # another device (the host stands in for one of two: the comparison is the devices', whatever they are)
    a, b = _marked(), _marked()
    b[0]._buffers["tsdf"] = torch.empty_like(b[1]["tsdf"], device="meta")
    with pytest.raises(SafError, match="different devices"):
        a[0].absorb(b[0])
    _assert_untouched(*a)
    # another lattice: an origin that differs in one float32 bit, another voxel size, another truncation distance
    moved = GRID.origin.clone().float()
    moved[1] = torch.nextafter(moved[1], torch.tensor(10.0))
    _refused(_marked(), _marked(origin=moved), "same lattice")
    _refused(_marked(), _marked(voxel_size=GRID.voxel_size * 2), "same lattice")
    _refused(_marked(), _marked(trunc=GRID.trunc * 1.5), "same lattice")
    # the same origin given in float64 IS the same lattice: it fails later, for the want of a device, not here
    with pytest.raises(SafError, match="no CPU fallback"):
        _cpu_module().absorb(_cpu_module(origin=GRID.origin.double()))
    # another layout
    _refused(_marked(), _marked(dim=16), "differ")
    _refused(_marked(), _marked(fdt=torch.float16), "differ")
    _refused(_marked(), _marked(seem=True), "differ")  # (classes and the rgb sampling)
    a, b = _marked(seem=True), _marked(seem=True)
    b[0]._buffers["labels_one_hot"] = b[1]["labels_one_hot"] = torch.zeros((12 * 10 * 14, 7), dtype=torch.int32)
    _refused(a, b, "differ")
    # SAF_SUM
    for which in (0, 1):
        pair = [_marked(), _marked()]
        pair[which][0].__dict__["accum_mode"] = _abi.SAF_SUM
        _refused(*pair, "running means")
        with pytest.raises(SafError, match="running means"):
            pair[0][0].absorb(pair[1][0], grow=False)


# ---- reconstruct_scene(lattice_of=...) ------------------------------------------------------------------------------------------
def test_scene_box_on_another_scenes_lattice_is_lattice_box_of_the_cloud_alone():
    from spatially_aware_ai_amd.clipfusion import scene_bounds
    from spatially_aware_ai_amd.scene import _scene_box

    base = _cpu_module(nvox=(12, 10, 14), index_offset=(-2, 3, 0))
    xyz = torch.from_numpy(np.random.default_rng(4).normal(size=(2000, 3)) * 0.2 + np.array([2.0, 0.0, -1.5])).float()
    origin, nvox, off = _scene_box(xyz, base.voxel_size, base.trunc, SimpleNamespace(fusion=base))
    want_off, want_n = lattice_box(base, xyz, union=False)
    assert off == want_off and tuple(int(v) for v in nvox) == want_n and all(v % 4 == 0 for v in want_n)
    assert torch.equal(torch.as_tensor(origin), torch.as_tensor(base.origin)), "the lattice's origin, not the cloud's"
    assert off != base.index_offset, "the cloud's own box, not a union with the base's"
    # the module built from it shares the base's voxel centres bit for bit wherever the boxes meet (test_carry_host.py)
    # ... and the default is scene_bounds, at the lattice's voxel 0
    o0, n0, off0 = _scene_box(xyz, base.voxel_size, base.trunc)
    o1, n1 = scene_bounds(xyz, base.voxel_size, base.trunc)
    assert torch.equal(o0, o1) and torch.equal(n0, n1) and off0 == (0, 0, 0)
    for vs, tr in ((base.voxel_size * 2, base.trunc), (base.voxel_size, base.trunc * 2)):
        with pytest.raises(SafError, match="lattice_of"):
            _scene_box(xyz, vs, tr, SimpleNamespace(fusion=base))
