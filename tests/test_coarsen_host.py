"""CPU: coarsening a fused volume by a whole factor (``coarsen``, ``coarsen_scene``; include/saf.h: saf_volume_coarsen) as far as it
can be checked without a GPU -- the NumPy restatement (tests/coarsen_reference.py) on itself, the mapping of boxes and lattices,
the refusals the library decides on the host, and ``coarsen()``'s own refusals.

The error bound used here and in test_coarsen_gpu.py, against the float64 weighted mean, with u = 2^-24: a coefficient
c_k = fl(fl(w_k) * fl(1 / fl(W))) carries up to three roundings, a product x_k * c_k one, the K - 1 sums one each on a partial sum
whose magnitude is at most sum |x_k| c_k <= max |x| (1 + O(u)); one more u covers the second-order terms:
|result - mean| <= (K + 4) u max_c |x_c|."""
import ctypes

import numpy as np
import pytest
import torch

from spatially_aware_ai_amd import _abi, _lib
from spatially_aware_ai_amd._lib import SafError
from spatially_aware_ai_amd.clipfusion import _axis_tables, coarse_lattice

import coarsen_reference as ref
from host_stubs import P, fake_volume
from test_absorb_host import FAR, GRID, _assert_untouched, _cpu_module, _marked

U = 2.0 ** -24
FACTORS = (2, 3, 4)


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _block(f, dim, rng, w, classes=0):
    """One block of f^3 fine voxels (a fine box of f x f x f at offset 0) whose children have the counts ``w`` on both sides."""
    n = (f, f, f)
    w = np.asarray(w, dtype=np.int32).reshape(n)
    v = {"tsdf": rng.standard_normal(n).astype(np.float32), "tsdf_weight": w.copy(), "weight": w.copy(),
         "rgb": rng.random(n + (3,)).astype(np.float32), "clip_feat": rng.standard_normal(n + (dim,)).astype(np.float32)}
    if classes:
        v["labels_one_hot"] = rng.integers(0, 50, n + (classes,)).astype(np.int32)
    return v


# ---- the restatement on itself ------------------------------------------------------------------------------------------------
def test_one_contributing_child_is_a_byte_copy_for_every_count():
    inexact = [w for w in range(1, 301) if np.float32(w) * (np.float32(1) / np.float32(w)) != np.float32(1)]
    assert inexact, "no count in 1 .. 300 for which w * fl(1 / w) is not 1: the copy case would prove nothing"
    rng = np.random.default_rng(1)
    for kind in ("f32", "bf16", "f16"):
        for f in FACTORS:
            # 300 blocks in a row along x; block i has one contributing child, of count i + 1
            n = (300 * f, f, f)
            child = rng.integers(0, f, (300, 3))
            at = (np.arange(300) * f + child[:, 0], child[:, 1], child[:, 2])
            w = np.zeros(n, np.int32)
            w[at] = np.arange(1, 301)
            v = {"tsdf": rng.standard_normal(n).astype(np.float32), "tsdf_weight": w.copy(), "weight": w.copy(),
                 "rgb": rng.random(n + (3,)).astype(np.float32), "clip_feat": rng.standard_normal(n + (5,)).astype(np.float32),
                 "labels_one_hot": rng.integers(0, 50, n + (3,)).astype(np.int32)}
            v["clip_feat"] = ref.narrow(v["clip_feat"], kind)
            out, inc = ref.coarsen(v, (0, 0, 0), f, kind)
            assert inc == (0, 300, 0, 300)
            for name in ("tsdf", "rgb", "clip_feat", "labels_one_hot"):
                assert np.array_equal(_bits(out[name][:, 0, 0]), _bits(v[name][at])), (name, f, kind)
            assert np.array_equal(out["weight"][:, 0, 0], np.arange(1, 301)) and np.array_equal(out["tsdf_weight"], out["weight"])


@pytest.mark.parametrize("f", FACTORS)
def test_a_constant_row_stays_the_constant_within_the_bound(f):
    rng = np.random.default_rng(2)
    for k in sorted({2, 3, f ** 3 // 2, f ** 3}):
        for const in (1.0, -3.7, 1e-3, 12345.678):
            counts = np.zeros(f ** 3, np.int32)
            counts[rng.choice(f ** 3, k, replace=False)] = rng.integers(1, 301, k)
            v = _block(f, 4, rng, counts)
            v["clip_feat"][:], v["rgb"][:], v["tsdf"][:] = const, const, const
            out, inc = ref.coarsen(v, (0, 0, 0), f)
            assert inc == (1, 0, 1, 0)
            c32 = np.float32(const)
            for name in ("clip_feat", "rgb", "tsdf"):
                err = np.abs(out[name].astype(np.float64) - np.float64(c32)).max()
                assert err <= (k + 4) * U * abs(float(c32)), (name, f, k, const, err)


def test_nothing_of_a_child_with_count_zero_reaches_the_output():
    rng = np.random.default_rng(3)
    for kind in ("f32", "bf16", "f16"):
        n, off, f = (7, 5, 9), (-3, 1, -2), 2
        draw = lambda: (rng.integers(0, 2, n) * rng.integers(1, 301, n)).astype(np.int32)
        v = {"tsdf": rng.standard_normal(n).astype(np.float32), "tsdf_weight": draw(), "weight": draw(),
             "rgb": rng.random(n + (3,)).astype(np.float32), "clip_feat": rng.standard_normal(n + (6,)).astype(np.float32),
             "labels_one_hot": rng.integers(0, 50, n + (4,)).astype(np.int32)}
        v["clip_feat"][v["weight"] == 0] = np.nan
        v["rgb"][v["weight"] == 0] = np.nan
        v["labels_one_hot"][v["weight"] == 0] = -(1 << 30)
        v["tsdf"][v["tsdf_weight"] == 0] = np.nan
        v["clip_feat"] = ref.narrow(v["clip_feat"], kind)
        out, inc = ref.coarsen(v, off, f, kind)
        k, kt = ref.child_counts(v, off, f)
        assert (k == 0).any() and (k == 1).any() and (k >= 2).any() and (kt == 0).any() and (kt >= 2).any()
        assert inc == (int((k >= 2).sum()), int((k == 1).sum()), int((kt >= 2).sum()), int((kt == 1).sum()))
        assert np.isfinite(ref.widen(out["clip_feat"], kind)).all() and np.isfinite(out["rgb"]).all() and np.isfinite(out["tsdf"]).all()
        assert (out["labels_one_hot"] >= 0).all()
        # labels: the exact sums; stored counts: the maxima; nothing where no child contributes
        lab = ref.children(np.where((v["weight"] > 0)[..., None], v["labels_one_hot"], 0), off, f).sum(-2)
        assert np.array_equal(out["labels_one_hot"], lab)
        assert np.array_equal(out["weight"], ref.children(v["weight"], off, f).max(-1))
        assert np.array_equal(out["tsdf_weight"], ref.children(v["tsdf_weight"], off, f).max(-1))
        for name in ("clip_feat", "rgb", "labels_one_hot"):
            assert int(np.abs(_bits(out[name])[k == 0]).max()) == 0, name
        assert int(np.abs(_bits(out["tsdf"])[kt == 0]).max()) == 0


@pytest.mark.parametrize("f", FACTORS)
def test_a_linear_tsdf_over_a_fully_observed_block_is_its_centre_value(f):
    rng = np.random.default_rng(4)
    g = rng.standard_normal(3)
    idx = np.stack(np.meshgrid(*[np.arange(f)] * 3, indexing="ij"), axis=-1).astype(np.float64)
    field = (idx @ g + 0.25).astype(np.float32)
    v = _block(f, 2, rng, np.full(f ** 3, 7, np.int32))
    v["tsdf"] = field
    out, _ = ref.coarsen(v, (0, 0, 0), f)
    centre = np.full(3, 0.5 * (f - 1)) @ g + 0.25
    bound = (f ** 3 + 4) * U * float(np.abs(field).max()) + U * float(np.abs(field).max())  # (the field itself was rounded to f32)
    assert abs(float(out["tsdf"][0, 0, 0]) - centre) <= bound
    # ... and the known bias: observed on one side only, the value is that side's, up to half a coarse voxel off
    v["tsdf_weight"][f // 2 + f % 2:] = 0
    low, _ = ref.coarsen(v, (0, 0, 0), f)
    assert abs(float(low["tsdf"][0, 0, 0]) - centre) > 0.1 * abs(g[0])


def test_restatement_agrees_with_the_float64_mean_within_the_bound():
    rng = np.random.default_rng(5)
    for f in FACTORS:
        n, off = (9, 6, 11), (-5, 3, -7)
        draw = lambda: (rng.integers(0, 2, n) * rng.integers(1, 301, n)).astype(np.int32)
        v = {"tsdf": rng.standard_normal(n).astype(np.float32), "tsdf_weight": draw(), "weight": draw(),
             "rgb": rng.random(n + (3,)).astype(np.float32), "clip_feat": rng.standard_normal(n + (16,)).astype(np.float32)}
        out, _ = ref.coarsen(v, off, f)
        w = ref.children(v["weight"], off, f)
        k = (w > 0).sum(-1)
        x = ref.children(v["clip_feat"], off, f)
        mean = ref.mean64(x, w)
        big = np.where((w > 0)[..., None], np.abs(x), 0).max(-2)
        m = k >= 2
        assert m.sum() > 10
        assert (np.abs(out["clip_feat"].astype(np.float64) - mean)[m] <= ((k + 4) * U)[m][:, None] * big[m]).all(), f


# ---- the mapping --------------------------------------------------------------------------------------------------------------
def test_mapping_of_boxes_with_offsets_of_both_signs():
    for f in FACTORS:
        for off, n in (((-5, 3, -7), (13, 10, 131)), ((0, 0, 0), (8, 8, 128)), ((-1, -4, 7), (1, 4, 2)), ((5, -9, 1), (3, 3, 3))):
            _, _, new_off, new_n = coarse_lattice(GRID.origin, GRID.voxel_size, off, n, f)
            assert (new_off, new_n) == ref.mapping(off, n, f)[:2]
            for a in range(3):
                fine = np.arange(off[a], off[a] + n[a])
                blocks = np.floor(fine / f).astype(np.int64)  # global coarse index I covers f I .. f I + f - 1
                assert new_off[a] == blocks.min() and new_n[a] == blocks.max() - blocks.min() + 1, (f, off, n, a)
    assert coarse_lattice(GRID.origin, GRID.voxel_size, (-5, 3, -7), (13, 10, 131), 2)[2:] == ((-3, 1, -4), (7, 6, 66))


def test_two_boxes_of_one_lattice_coarsen_onto_one_lattice():
    for f in FACTORS:
        a = coarse_lattice(GRID.origin, GRID.voxel_size, (-5, 3, -7), (13, 10, 31), f)
        b = coarse_lattice(GRID.origin, GRID.voxel_size, (40, -17, 2), (9, 9, 9), f)
        assert torch.equal(a[0], b[0]) and a[1] == b[1] == f * GRID.voxel_size
        assert a[0].dtype == GRID.origin.dtype
        want = GRID.origin.double() + 0.5 * (f - 1) * float(GRID.voxel_size)
        assert torch.equal(a[0], want.to(GRID.origin.dtype))
    # the container and dtype the origin came in
    o = coarse_lattice(np.array([0.5, 1.0, -2.0], dtype=np.float64), 0.1, (0, 0, 0), (4, 4, 4), 2)[0]
    assert isinstance(o, np.ndarray) and o.dtype == np.float64 and np.array_equal(o, np.array([0.55, 1.05, -1.95]))
    o = coarse_lattice([0.5, 1.0, -2.0], 0.1, (0, 0, 0), (4, 4, 4), 3)[0]
    assert isinstance(o, list) and o == [0.6, 1.1, -1.9]


@pytest.mark.parametrize("f", FACTORS)
def test_axis_tables_of_the_coarse_box_are_a_fresh_modules(f):
    off, n = (-5, 3, -7), (13, 10, 31)
    origin, vs, new_off, new_n = coarse_lattice(GRID.origin, GRID.voxel_size, off, n, f)
    fresh = _cpu_module(nvox=new_n, index_offset=new_off, origin=origin, voxel_size=f * GRID.voxel_size)
    ax = _axis_tables(origin, vs, new_n, new_off)
    fine = _axis_tables(GRID.origin, GRID.voxel_size, n, off)
    for a, name in enumerate(("axis_x", "axis_y", "axis_z")):
        assert torch.equal(ax[a].view(torch.int32), fresh._buffers[name].view(torch.int32)), name
        # a coarse centre is the centre of its block: the mean of its children's centres, within the tables' own rounding
        lead = off[a] - f * new_off[a]
        for i in range(new_n[a]):
            kids = [j for j in range(f * i - lead, f * i - lead + f)]
            if kids[0] >= 0 and kids[-1] < n[a]:
                assert abs(float(ax[a][i]) - float(fine[a][kids].double().mean())) <= 4 * 2.0 ** -23 * max(1.0, abs(float(ax[a][i])))


# ---- the entry point's refusals, decided before anything is launched ----------------------------------------------------------
# (every call below is refused: a call that passed the checks would launch the kernel on the stand-in pointers)
def _pair(n_src=8, n_dst=4, dim=8, dtype=_abi.SAF_F32, classes=0):
    src = fake_volume(n_src, dim, dtype, n_classes=classes, labels_one_hot=P if classes else None)
    dst = fake_volume(n_dst, dim, dtype, n_classes=classes)
    for name in ("tsdf", "tsdf_weight", "weight", "rgb", "clip_feat") + (("labels_one_hot",) if classes else ()):
        setattr(dst, name, FAR)
    return src, dst


def _coarsen(src, dst, f=2, off=(0, 0, 0), counts=None):
    l = _lib.lib()
    rc = l.saf_volume_coarsen(None if src is None else ctypes.byref(src), None if dst is None else ctypes.byref(dst), f, off[0], off[1],
                              off[2], counts, None)
    assert rc != 0, "a call on stand-in pointers passed the checks"
    return rc, l.saf_last_error().decode()


def test_coarsen_refuses_nulls_and_bad_sizes():
    src, dst = _pair()
    assert _coarsen(None, dst)[0] == _abi.SAF_E_INVALID and _coarsen(src, None)[0] == _abi.SAF_E_INVALID
    for which in (0, 1):
        for name in ("tsdf", "tsdf_weight", "weight", "rgb", "clip_feat"):
            pair = _pair()
            setattr(pair[which], name, None)
            rc, msg = _coarsen(*pair)
            assert rc == _abi.SAF_E_INVALID and "NULL" in msg, (which, name)
        for name in ("nx", "ny", "nz"):
            for bad in (0, -3):
                pair = _pair()
                setattr(pair[which], name, bad)
                assert _coarsen(*pair)[0] == _abi.SAF_E_INVALID, (which, name, bad)
        pair = _pair(classes=143)
        pair[which].labels_one_hot = None
        assert _coarsen(*pair)[0] == _abi.SAF_E_INVALID
        pair = _pair()
        pair[which].nx, pair[which].ny, pair[which].nz = 2048, 1024, 1024  # 2^31 voxels
        rc, msg = _coarsen(*pair)
        assert rc == _abi.SAF_E_INVALID and "2^31" in msg
        pair = _pair()
        pair[which].feat_dtype = 7
        assert _coarsen(*pair)[0] == _abi.SAF_E_INVALID
    assert _coarsen(*_pair(dim=0))[0] == _abi.SAF_E_INVALID


def test_coarsen_refuses_volumes_that_differ_or_share_bytes():
    for change in (dict(feat_dim=16), dict(feat_dtype=_abi.SAF_BF16), dict(n_classes=143, labels_one_hot=FAR)):
        src, dst = _pair()
        for k, v in change.items():
            setattr(dst, k, v)
        rc, msg = _coarsen(src, dst)
        assert rc == _abi.SAF_E_INVALID and "differ" in msg, change
    sizes = {"tsdf": 4, "tsdf_weight": 4, "weight": 4, "rgb": 12, "clip_feat": 4 * 8, "labels_one_hot": 4 * 143}
    for name, per_voxel in sizes.items():
        for delta in (0, 8 ** 3 * per_voxel - 4, -(4 ** 3 * per_voxel - 4)):
            src, dst = _pair(classes=143)
            setattr(src, name, FAR // 2)
            setattr(dst, name, FAR // 2 + delta)
            rc, msg = _coarsen(src, dst)
            assert rc == _abi.SAF_E_INVALID and "overlaps its source" in msg, (name, delta)


def test_coarsen_refuses_rows_that_are_not_aligned_to_their_element():
    src, dst = _pair()
    dst.clip_feat = FAR + 2
    rc, msg = _coarsen(src, dst)
    assert rc == _abi.SAF_E_INVALID and "aligned" in msg
    src, dst = _pair(dtype=_abi.SAF_F16)
    src.clip_feat = P + 1
    rc, msg = _coarsen(src, dst)
    assert rc == _abi.SAF_E_INVALID and "aligned" in msg
    src, dst = _pair(classes=143)
    dst.labels_one_hot = FAR + 2
    rc, msg = _coarsen(src, dst)
    assert rc == _abi.SAF_E_INVALID and "aligned" in msg


def test_coarsen_refuses_other_factors_and_a_destination_of_another_size():
    for f in (-2, 0, 1, 5, 8):
        rc, msg = _coarsen(*_pair(), f=f)
        assert rc == _abi.SAF_E_INVALID and "factor" in msg, f
    # 8 fine voxels per axis: 4 coarse ones at offset 0 -- with f = 2
    for f, off, n_dst in ((2, (0, 0, 0), 5), (2, (0, 0, 0), 3), (2, (1, 0, 0), 4), (2, (0, -1, 0), 4), (2, (0, 0, 3), 4), (3, (0, 0, 0), 4),
                          (4, (0, 0, 0), 4), (4, (-1, -1, -1), 2), (3, (0, 0, 0), 2)):
        want = ref.mapping(off, (8, 8, 8), f)[1]
        assert want != (n_dst,) * 3, "the case would pass the check"
        rc, msg = _coarsen(*_pair(n_dst=n_dst), f=f, off=off)
        assert rc == _abi.SAF_E_INVALID and "coarsens by" in msg, (f, off, n_dst)


def test_coarsen_takes_running_means_only():
    for which in (0, 1):
        pair = _pair()
        pair[which].accum_mode = _abi.SAF_SUM
        rc, msg = _coarsen(*pair)
        assert rc == _abi.SAF_E_UNSUPPORTED and "running means" in msg, which


# ---- coarsen()'s own refusals ---------------------------------------------------------------------------------------------------
def _refused(fz_snap, match, factor=2):
    fz, snap = fz_snap
    lattice = (fz.origin, fz.voxel_size, fz.trunc)
    box = (fz.index_offset, tuple(int(v) for v in fz.nvox))
    with pytest.raises(SafError, match=match):
        fz.coarsen(factor)
    _assert_untouched(fz, snap, box)
    assert fz.origin is lattice[0] and fz.voxel_size == lattice[1] and fz.trunc == lattice[2]


def test_coarsen_refuses_slabs_stripes_poisoned_modules_sums_and_other_factors_and_leaves_the_volume_alone():
    _refused(_marked(nvox=(8, 10, 14), x_planes=[0, 1, 2, 3, 8, 9, 10, 11]), "x_planes")
    m = _marked()
    m[0]._shard_stripes = [(0, 100)]
    _refused(m, "stripes")
    m = _marked()
    m[0].__dict__["_poisoned"] = "a flush failed"
    _refused(m, "a flush failed")
    m[0].__dict__["_poisoned"] = None
    m = _marked()
    m[0].__dict__["accum_mode"] = _abi.SAF_SUM
    _refused(m, "running means")
    for factor in (1, 5, 0, -2, 2.0, "2", None, True, np.float32(2)):
        _refused(_marked(), "factor", factor)
    # a well-formed call fails later, for the want of a device, with the volume as it was
    _refused(_marked(), "no CPU fallback", 2)
    _refused(_marked(seem=True), "no CPU fallback", 4)


def test_the_package_exports_the_record():
    import spatially_aware_ai_amd as pkg
    from spatially_aware_ai_amd.clipfusion import GridCoarsen
    from spatially_aware_ai_amd.scene import coarsen_scene  # noqa: F401

    assert pkg.GridCoarsen is GridCoarsen and "GridCoarsen" in pkg.__all__
    fields = set(GridCoarsen.__dataclass_fields__)
    assert {"factor", "old_origin", "origin", "old_voxel_size", "voxel_size", "old_index_offset", "index_offset", "old_nvox", "nvox",
            "rows_blended", "rows_copied", "tsdf_blended", "tsdf_copied"} <= fields
