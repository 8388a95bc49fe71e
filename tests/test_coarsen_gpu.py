"""GPU: a fused volume coarsened by a whole factor (``coarsen``; include/saf.h: saf_volume_coarsen, csrc/saf_coarsen.hip).

(a), (b): the device pass against its NumPy restatement (tests/coarsen_reference.py) on random buffers, byte for byte, and against
the float64 weighted mean within the bound derived in tests/test_coarsen_host.py: (K + 4) 2^-24 max_c |x_c|, plus one narrowing
for 16-bit rows.  Rounding a to the nearest value y of p significant bits errs by at most half a unit in y's last place, 2^(e - p)
for 2^e <= |y| < 2^(e + 1): at most 2^-p |y|, with p = 8 for bfloat16 (7 stored bits and the hidden one) and p = 11 for float16
-- 2^-8 and 2^-11 of the result's magnitude (2^-9 and 2^-12, half of that, are exceeded by the NumPy restatement alone on every
16-bit case below: a result just above a power of two is off by up to 2^-p of itself) -- and, for a float16 result below 2^-14,
half the subnormal spacing, 2^-25.
(c): ``coarsen(2)`` twice against ``coarsen(4)``.  The stored count of a coarse voxel is the MAXIMUM of its children's counts, so
the second coarsening weighs a 2-block by its largest count, not by the sum of its counts: the nested mean is the flat mean of
``coarsen(4)`` exactly where every contributing 2-block of a 4-block has the same sum / max ratio -- the volume of this case: one count
per 4-block, 2-blocks either fully observed or empty.  Labels and stored counts agree on any volume, and that is checked on random
counts too, where the means are held to the float64 NESTED mean.
(d): coarsening commutes with ``move_grid`` on block-aligned boxes, bit for bit.  (e), (f): fusion goes on at the coarse size, and
the module's other calls work; volumes of different voxel sizes joined.  (g): stale rows, queued frames.  (h): ``coarsen_scene``."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from spatially_aware_ai_amd import _abi
from spatially_aware_ai_amd import synthetic as syn
from spatially_aware_ai_amd._lib import SafError, check, lib
from spatially_aware_ai_amd.clipfusion import coarse_lattice

import absorb_reference as aref
import coarsen_reference as ref
from test_absorb_gpu import KIND, KIND_OF, _grids, _np_bits, _raw, _snapshot, _stale
from test_carry_gpu import BOX_A, GRID, H, NAMES, TORCH_DT, W, _bits, _descriptor, _fuse, _module, _names, \
    _one_by_one, _scan, _sentinel_destination, _to_device

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NARROW = {"f32": (0.0, 0.0), "bf16": (2.0 ** -8, 0.0), "f16": (2.0 ** -11, 2.0 ** -25)}  # (of the result, absolute)
BIG = (1 << 24) + 1  # a count that (float) rounds: to even, 2^24
LABEL_POISON = -(1 << 30)


# ---- (a) the pass on random buffers -------------------------------------------------------------------------------------------
def _block_children(blk, f, lead, n):
    """Flat fine indices of the children of coarse voxel ``blk`` that lie inside the fine box ``n``, in ascending order."""
    out = []
    for c in np.ndindex(f, f, f):
        p = [f * blk[a] - lead[a] + c[a] for a in range(3)]
        if all(0 <= p[a] < n[a] for a in range(3)):
            out.append(int(np.ravel_multi_index(p, n)))
    return out


def _random_source(n, off, f, dim, dt, classes, rng):
    """CPU tensors of a fine volume.  Both count arrays are drawn independently from {0, 1 .. 300}, about half zeros; the first
    blocks with all f^3 children inside the box are forced through K = f^3, 2 (one count 2^24 + 1), 1 and 0 on both sides (the TSDF
    side in reverse order).  Then the poison: whatever belongs to a child whose count is 0 is NaN (labels: a poison value).
    Returns the volume and whether the box has four such blocks."""
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    nv = int(np.prod(n))
    draw = lambda: torch.from_numpy((rng.integers(0, 2, nv) * rng.integers(1, 301, nv)).astype(np.int32))
    v = {"tsdf": torch.randn(nv, generator=g), "tsdf_weight": draw(), "weight": draw(), "rgb": torch.rand(nv, 3, generator=g),
         "clip_feat": torch.randn(nv, dim, generator=g).to(TORCH_DT[dt])}
    if classes:
        v["labels_one_hot"] = torch.from_numpy(rng.integers(0, 50, (nv, classes)).astype(np.int32))
    _, new_n, lead = ref.mapping(off, n, f)
    full = [b for b in np.ndindex(*new_n) if len(_block_children(b, f, lead, n)) == f ** 3][:4]
    forced = len(full) == 4
    if forced:
        plans = [lambda k: [7 + (j % 5) for j in range(k)], lambda k: [BIG, 3] + [0] * (k - 2), lambda k: [0] * (k - 1) + [9],
                 lambda k: [0] * k]
        for j, blk in enumerate(full):
            kids = torch.tensor(_block_children(blk, f, lead, n))
            v["weight"][kids] = torch.tensor(plans[j](f ** 3), dtype=torch.int32)
            v["tsdf_weight"][kids] = torch.tensor(plans[3 - j](f ** 3), dtype=torch.int32)
    v["clip_feat"][v["weight"] == 0] = float("nan")
    v["rgb"][v["weight"] == 0] = float("nan")
    v["tsdf"][v["tsdf_weight"] == 0] = float("nan")
    if classes:
        v["labels_one_hot"][v["weight"] == 0] = LABEL_POISON
    return v, forced


def _assert_within_the_float64_bound(got, src, off, f, kind):
    """Every blended value against the float64 weighted mean of its contributing children."""
    for name, side in (("clip_feat", "weight"), ("rgb", "weight"), ("tsdf", "tsdf_weight")):
        w = ref.children(src[side], off, f)
        k = (w > 0).sum(-1)
        x = src[name][..., None] if name == "tsdf" else src[name]
        x = ref.children(aref.widen(x, kind) if name == "clip_feat" else x, off, f)
        out = got[name][..., None] if name == "tsdf" else got[name]
        out = (aref.widen(out, kind) if name == "clip_feat" else out).astype(np.float64)
        m = k >= 2
        mean = ref.mean64(x, w)[m]
        big = np.where((w > 0)[..., None], np.abs(x), 0).max(-2)[m]
        bound = ((k + 4) * U)[m][:, None] * big
        if name == "clip_feat":
            bound = bound + NARROW[kind][0] * np.abs(out[m]) + NARROW[kind][1]
        assert m.any() and (np.abs(out[m] - mean) <= bound).all(), f"{name}: a blended value is further from the float64 mean than its bound"


M2, M3, M4 = (6, 6, 128), (6, 6, 192), (6, 6, 257)  # at offset (-5, 7, -7): partial blocks on all six faces, 65 coarse voxels along z
OFF = (-5, 7, -7)
PASS_CASES = [
    # factor, fine box, its offset, D, dtype, classes, misaligned (0 no, 1 destination, 2 source), coarse voxels along z
    pytest.param(2, M2, OFF, 512, _abi.SAF_F32, 143, 0, 65, id="f2-D512-f32-labels"),
    pytest.param(2, M2, OFF, 512, _abi.SAF_BF16, 0, 0, 65, id="f2-D512-bf16"),
    pytest.param(2, M2, OFF, 512, _abi.SAF_F16, 143, 0, 65, id="f2-D512-fp16-labels"),
    pytest.param(3, M3, OFF, 512, _abi.SAF_F32, 0, 0, 65, id="f3-D512-f32"),
    pytest.param(3, M3, OFF, 512, _abi.SAF_BF16, 143, 0, 65, id="f3-D512-bf16-labels"),
    pytest.param(3, M3, OFF, 512, _abi.SAF_F16, 0, 0, 65, id="f3-D512-fp16"),
    pytest.param(4, M4, OFF, 512, _abi.SAF_F32, 143, 0, 65, id="f4-D512-f32-labels"),
    pytest.param(4, M4, OFF, 512, _abi.SAF_BF16, 0, 0, 65, id="f4-D512-bf16"),
    pytest.param(4, M4, OFF, 512, _abi.SAF_F16, 143, 0, 65, id="f4-D512-fp16-labels"),
    pytest.param(2, (8, 8, 128), (0, 0, 0), 6, _abi.SAF_F32, 143, 0, 64, id="f2-aligned-box-D6-f32-24-byte-rows-labels"),
    pytest.param(3, (7, 6, 189), (2, -4, 0), 512, _abi.SAF_F32, 0, 1, 63, id="f3-63-along-z-D512-f32-destination-off-16-bytes"),
    pytest.param(4, (9, 9, 3), (-5, 7, -3), 12, _abi.SAF_F16, 143, 2, 1, id="f4-one-along-z-D12-fp16-24-byte-rows-source-off-16-bytes"),
    pytest.param(2, (13, 10, 131), (-5, 3, -7), 7, _abi.SAF_BF16, 143, 0, 66, id="f2-D7-bf16-14-byte-rows-labels"),
    pytest.param(2, M2, OFF, 512, _abi.SAF_BF16, 143, 1, 65, id="f2-D512-bf16-destination-off-16-bytes"),
    pytest.param(4, (13, 10, 131), (-5, 3, -7), 8, _abi.SAF_F32, 0, 2, 33, id="f4-D8-f32-source-off-16-bytes"),
]


@pytest.mark.parametrize("f,n,off,dim,dt,classes,misaligned,nz", PASS_CASES)
def test_pass_equals_its_restatement_and_touches_nothing_else(f, n, off, dim, dt, classes, misaligned, nz):
    kind = KIND[dt]
    rng = np.random.default_rng(abs(hash((f, n, off, dim, dt))) % (1 << 32))
    new_off, new_n, lead = ref.mapping(off, n, f)
    assert new_n[2] == nz
    if n in (M2, M3, M4):
        assert all(lead[a] != 0 and (off[a] + n[a]) % f != 0 for a in range(3)), "the case has no partial blocks on some face"
    src, forced = _random_source(n, off, f, dim, dt, classes, rng)
    src_g = _grids(src, n, kind)
    k, kt = ref.child_counts(src_g, off, f)
    if n != (9, 9, 3):  # (one block along z, cut on both sides: no block has all its children)
        assert forced
        for kk in (k, kt):  # a condition of the test: every case of the statement, on both sides
            assert (kk == 0).any() and (kk == 1).any() and (kk == 2).any() and (kk == f ** 3).any()
        assert (src_g["weight"] == BIG).any() and (src_g["tsdf_weight"] == BIG).any()
    dst = _sentinel_destination(src, new_n)
    before = _grids(dst, new_n, kind)
    want, inc = ref.coarsen(src_g, off, f, kind, dst=before)
    s_dev, d_dev = _to_device(src, misaligned == 2), _to_device(dst, misaligned == 1)
    counts = torch.tensor([5, 7, 11, 13], dtype=torch.int64, device="cuda")
    vs, vd = _descriptor(s_dev, n, dim, dt), _descriptor(d_dev, new_n, dim, dt)
    check(lib().saf_volume_coarsen(C.byref(vs), C.byref(vd), f, off[0], off[1], off[2], counts.data_ptr(), None), "saf_volume_coarsen")
    torch.cuda.synchronize()
    got = _grids(d_dev, new_n, kind)
    for name in want:
        assert np.array_equal(_np_bits(got[name]), _np_bits(want[name])), f"{name} differs from the restatement"
    # said once more without the restatement's help: the rows of coarse voxels without a contributing child keep their pattern,
    # the small fields are written everywhere -- zero where nothing contributes ...
    for name in ("clip_feat",) + (("labels_one_hot",) if classes else ()):
        assert np.array_equal(_np_bits(got[name])[k == 0], _np_bits(before[name])[k == 0]), f"{name}: a row without a child was written"
    assert not _np_bits(got["rgb"])[k == 0].any() and not got["weight"][k == 0].any()
    assert not _np_bits(got["tsdf"])[kt == 0].any() and not got["tsdf_weight"][kt == 0].any()
    # ... nothing poisoned was read ...
    assert np.isfinite(aref.widen(got["clip_feat"], kind)[k > 0]).all() and np.isfinite(got["rgb"]).all() and np.isfinite(got["tsdf"]).all()
    if classes:
        assert (got["labels_one_hot"][k > 0] >= 0).all()
    # ... the stored counts are the maxima, the labels the sums ...
    assert np.array_equal(got["weight"], ref.children(src_g["weight"], off, f).max(-1))
    assert np.array_equal(got["tsdf_weight"], ref.children(src_g["tsdf_weight"], off, f).max(-1))
    assert counts.tolist() == [5 + inc[0], 7 + inc[1], 11 + inc[2], 13 + inc[3]], "the counters are added to, exactly"
    assert inc == (int((k >= 2).sum()), int((k == 1).sum()), int((kt >= 2).sum()), int((kt == 1).sum()))
    _assert_within_the_float64_bound(got, src_g, off, f, kind)
    # ... and the source is only read
    for name, t in src.items():
        assert torch.equal(_bits(s_dev[name]).cpu(), _bits(t)), f"the source's {name} changed"


# ---- (b) rows beyond 4 GB in the source ----------------------------------------------------------------------------------------
def test_pass_addresses_rows_beyond_4_gigabytes():
    dim, n, f = 8192, (64, 64, 66), 2
    new_n = (32, 32, 33)
    ns, nd = int(np.prod(n)), int(np.prod(new_n))
    assert ns * dim * 2 > 1 << 32
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(5)
    zeros = lambda k, *shape, dtype=torch.float32: torch.zeros((k,) + shape, dtype=dtype, device=dev)
    src = {"tsdf": zeros(ns), "tsdf_weight": zeros(ns, dtype=torch.int32), "weight": zeros(ns, dtype=torch.int32), "rgb": zeros(ns, 3),
           "clip_feat": torch.empty((ns, dim), dtype=torch.bfloat16, device=dev)}  # (untouched rows: whatever the allocator left)
    dst = {"tsdf": zeros(nd), "tsdf_weight": zeros(nd, dtype=torch.int32), "weight": zeros(nd, dtype=torch.int32), "rgb": zeros(nd, 3),
           "clip_feat": zeros(nd, dim, dtype=torch.bfloat16)}
    blocks = np.arange(nd - 100, nd)  # the last hundred coarse voxels: K = 1, 2, 8 in turn
    plans = ([0, 0, 0, 5, 0, 0, 0, 0], [3, 0, 0, 0, 0, 0, 200, 0], [1, 2, 3, 4, 5, 6, 7, 8])
    mini = {"weight": np.zeros((200, 2, 2), np.int32), "clip_feat": np.zeros((200, 2, 2, dim), np.int16)}
    kids_all, w_all = [], []
    for j, b in enumerate(blocks):
        kids = _block_children(np.unravel_index(b, new_n), f, (0, 0, 0), n)
        kids_all += kids
        w_all += plans[j % 3]
        mini["weight"][2 * j:2 * j + 2] = np.asarray(plans[j % 3], np.int32).reshape(2, 2, 2)
    kids_t, w_t = torch.tensor(kids_all, device=dev), torch.tensor(w_all, dtype=torch.int32, device=dev)
    assert int(kids_t[w_t > 0].min()) * dim * 2 > 1 << 32, "the rows read do not lie beyond 4 GB"
    rows = torch.randn((len(kids_all), dim), generator=g, device=dev).to(torch.bfloat16)
    src["weight"][kids_t] = w_t
    src["clip_feat"][kids_t[w_t > 0]] = rows[w_t > 0]
    mini["clip_feat"][:] = rows.cpu().view(torch.int16).numpy().reshape(100, 2, 2, 2, dim).reshape(200, 2, 2, dim)
    for name in ("tsdf", "rgb"):
        mini[name] = np.zeros((200, 2, 2) + ((3,) if name == "rgb" else ()), np.float32)
    mini["tsdf_weight"] = np.zeros((200, 2, 2), np.int32)
    want, inc = ref.coarsen(mini, (0, 0, 0), f, "bf16")
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    vs, vd = _descriptor(src, n, dim, _abi.SAF_BF16), _descriptor(dst, new_n, dim, _abi.SAF_BF16)
    check(lib().saf_volume_coarsen(C.byref(vs), C.byref(vd), f, 0, 0, 0, counts.data_ptr(), None), "saf_volume_coarsen")
    torch.cuda.synchronize()
    there = torch.from_numpy(blocks).to(dev)
    got = dst["clip_feat"].index_select(0, there).cpu().view(torch.int16).numpy()
    assert np.array_equal(got, want["clip_feat"][:, 0, 0])
    assert np.array_equal(dst["weight"][there].cpu().numpy(), want["weight"][:, 0, 0]) and int(dst["weight"].sum()) == int(want["weight"].sum())
    assert counts.tolist() == [inc[0], inc[1], 0, 0] and inc[0] == 66 and inc[1] == 34
    untouched = torch.ones(nd, dtype=torch.bool, device=dev)
    untouched[there] = False
    sample = torch.cat((torch.arange(0, nd, 97, device=dev), torch.arange(nd - 300, nd, device=dev)))
    sample = sample[untouched[sample]]
    assert sample.numel() > 400 and int(_bits(dst["clip_feat"].index_select(0, sample)).abs().max()) == 0, "an untouched row was written"


# ---- (c) - (h): modules -------------------------------------------------------------------------------------------------------
def _module_at(scan, origin, voxel_size, box, seem=True, fdt=torch.float32, defer=False, first_frame=0):
    """test_carry_gpu's ``_module`` on any lattice."""
    from spatially_aware_ai_amd import ClipFusion, ClipSeemFusion

    clip, seg = syn.ReplayClip(scan), syn.ReplaySeg(scan)
    clip.calls = seg.calls = first_frame
    off, n = box
    if seem:
        return ClipSeemFusion(origin, voxel_size, torch.tensor(n), GRID.trunc, False, 16, 8, clip, seg, feat_dtype=fdt,
                              defer_frames=defer, index_offset=off).cuda()
    return ClipFusion(origin, voxel_size, torch.tensor(n), GRID.trunc, False, clip, None, 16, 8, feat_dtype=fdt, defer_frames=defer,
                      index_offset=off).cuda()


def _load(fz, vol):
    """A module's buffers filled from grids (coarsen_reference's layout; 16-bit rows as bit patterns)."""
    for name, a in vol.items():
        t = fz._buffers[name]
        src = torch.from_numpy(np.ascontiguousarray(a)).reshape(t.shape[0], *a.shape[3:])
        if name == "clip_feat" and t.dtype != torch.float32:
            src = src.view(t.dtype)
        t.copy_(src.reshape(t.shape))
    return fz


def _random_volume(n, dim, rng, classes=143, weights=None):
    """Grids of a volume as a module holds it: zero wherever the count is 0."""
    draw = lambda: (rng.integers(0, 2, n) * rng.integers(1, 301, n)).astype(np.int32)
    w, tw = (draw(), draw()) if weights is None else (weights.copy(), weights.copy())
    v = {"tsdf": rng.standard_normal(n).astype(np.float32) * (tw > 0), "tsdf_weight": tw, "weight": w,
         "rgb": rng.random(n + (3,)).astype(np.float32) * (w > 0)[..., None],
         "clip_feat": rng.standard_normal(n + (dim,)).astype(np.float32) * (w > 0)[..., None]}
    if classes:
        v["labels_one_hot"] = rng.integers(0, 50, n + (classes,)).astype(np.int32) * (w > 0)[..., None]
    return {k: np.ascontiguousarray(a.astype(np.float32) if a.dtype == np.float64 else a) for k, a in v.items()}


def _box(fz):
    return fz.index_offset, tuple(int(v) for v in fz.nvox)


def test_coarsen_twice_by_2_against_once_by_4():
    dim, box = 64, ((-8, 4, -4), (8, 12, 16))
    scan = _scan(dim, 11)
    rng = np.random.default_rng(7)
    # one count per 4-block (some 4-blocks empty), 2-blocks fully observed or empty: the nested mean IS the flat mean
    w4 = (rng.integers(0, 4, (2, 3, 4)) > 0) * rng.integers(1, 301, (2, 3, 4))
    on2 = rng.integers(0, 3, (4, 6, 8)) > 0
    w = (np.kron(w4, np.ones((4, 4, 4), np.int64)) * np.kron(on2, np.ones((2, 2, 2), np.int64))).astype(np.int32)
    structured = _random_volume(box[1], dim, rng, weights=w)
    general = _random_volume(box[1], dim, rng)
    for vol, flat in ((structured, True), (general, False)):
        once, twice = _load(_module(scan, box), vol), _load(_module(scan, box), vol)
        rec4 = once.coarsen(4)
        rec2 = twice.coarsen(2)
        assert (rec2.index_offset, rec2.nvox) == ((-4, 2, -2), (4, 6, 8)) and float(rec2.voxel_size) == 2 * float(GRID.voxel_size)
        half = _grids(_snapshot(twice), rec2.nvox, "f32")
        rec22 = twice.coarsen(2)
        assert (rec4.index_offset, rec4.nvox) == (rec22.index_offset, rec22.nvox) == _box(once) == _box(twice) == ((-2, 1, -1), (2, 3, 4))
        assert float(once.voxel_size) == float(twice.voxel_size) == 4 * float(GRID.voxel_size)
        o4 = torch.as_tensor(once.origin).double()
        assert float((o4 - torch.as_tensor(twice.origin).double()).abs().max()) <= 2.0 ** -22 * float(o4.abs().max()), \
            "origin + 0.5 vs + 0.5 (2 vs) and origin + 1.5 vs differ by more than their float32 roundings"
        a, b = _grids(_snapshot(once), rec4.nvox, "f32"), _grids(_snapshot(twice), rec4.nvox, "f32")
        # labels: the sums; stored counts: the max of the maxima -- on any volume
        for name in ("labels_one_hot", "weight", "tsdf_weight"):
            assert np.array_equal(a[name], b[name]), f"{name}: twice by 2 differs from once by 4"
        assert int((a["weight"] > 0).sum()) > 5 and int((a["weight"] == 0).sum()) >= (1 if flat else 0)
        for name, side in (("clip_feat", "weight"), ("rgb", "weight"), ("tsdf", "tsdf_weight")):
            x = vol[name][..., None] if name == "tsdf" else vol[name]
            w4c, x4 = ref.children(vol[side], box[0], 4), ref.children(x, box[0], 4)
            k4 = (w4c > 0).sum(-1)
            big = np.where((w4c > 0)[..., None], np.abs(x4), 0).max(-2)
            bound4 = ((k4 + 4) * U)[..., None] * big
            # the second pass's children are the first pass's results, its counts the first pass's maxima
            w2a = ref.children(vol[side], box[0], 2)
            k2a = ref.children((w2a > 0).sum(-1), rec2.index_offset, 2)
            xh = half[name][..., None] if name == "tsdf" else half[name]
            w2b = ref.children(half[side], rec2.index_offset, 2)
            k2b = (w2b > 0).sum(-1)
            inner = ((np.where(w2b > 0, k2a, 0).max(-1) + 4) * U)[..., None] * big
            outer = ((k2b + 4) * U)[..., None] * big
            ga = (a[name][..., None] if name == "tsdf" else a[name]).astype(np.float64)
            gb = (b[name][..., None] if name == "tsdf" else b[name]).astype(np.float64)
            m = k4 >= 2
            flat_mean = ref.mean64(x4, w4c)
            assert (np.abs(ga - flat_mean)[m] <= bound4[m]).all(), f"{name}: once by 4 against the float64 mean"
            if flat:
                assert (np.abs(gb - flat_mean)[m] <= (inner + outer)[m]).all(), f"{name}: twice by 2 against the float64 mean"
            # the float64 nested mean: float64 means of the 2-blocks, weighed by the maxima
            mean2 = np.nan_to_num(ref.mean64(ref.children(x, box[0], 2), w2a))
            nested = ref.mean64(ref.children(mean2, rec2.index_offset, 2), w2b)
            m2 = k2b >= 1
            assert (np.abs(gb - nested)[m2] <= (inner + outer)[m2]).all(), f"{name}: twice by 2 against the float64 nested mean"


@pytest.mark.parametrize("f", [2, 3, 4])
def test_coarsen_commutes_with_the_move_bit_for_bit(f):
    dim = 64
    scan = _scan(dim, 11)
    rng = np.random.default_rng(11 + f)
    box = ((-2 * f, f, 0), (4 * f, 3 * f, 5 * f))  # block-aligned
    to = ((-f, -f, 2 * f), (4 * f, 4 * f, 4 * f))  # another block-aligned box of the fine lattice: drops, keeps and adds blocks
    vol = _random_volume(box[1], dim, rng)
    a, b = _load(_module(scan, box), vol), _load(_module(scan, box), vol)
    a.coarsen(f)
    move_a = a.move_grid(tuple(o // f for o in to[0]), tuple(n // f for n in to[1]))
    b.move_grid(*to)
    rec_b = b.coarsen(f)
    assert _box(a) == _box(b) == (rec_b.index_offset, rec_b.nvox) and int(move_a.rows_carried) > 0 and int(move_a.rows_dropped) > 0
    assert torch.equal(torch.as_tensor(a.origin), torch.as_tensor(b.origin)) and a.voxel_size == b.voxel_size
    for name in ("axis_x", "axis_y", "axis_z"):
        assert torch.equal(_bits(a._buffers[name]), _bits(b._buffers[name])), name
    assert int((a.weight > 0).sum()) > 10 and int((a.weight == 0).sum()) > 10
    for name in NAMES:
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), f"{name}: coarsen then move differs from move then coarsen"


def _fused_then_coarsened(dim, m, n, seem, fdt=torch.float32):
    """Frames 1..m, ``coarsen(2)``, frames m+1..n; and a fresh module on the coarse lattice, loaded with the restatement of the first
    volume and fed the same later frames.  Returns (module, fresh module, record, restatement's counters)."""
    scan = _scan(dim, n)
    fr = scan.frames
    kind = KIND_OF[fdt]
    fz = _fuse(_module(scan, BOX_A, seem, fdt), fr[:m], seem)
    fine = _grids(_snapshot(fz, seem), BOX_A[1], kind)
    stats_ptr, clip = fz._buffers["fuse_stats"].data_ptr(), fz.clip
    fz.voxel_obj_idx = torch.zeros(fz._buffers["weight"].numel(), dtype=torch.int32, device="cuda")
    fz.objects_segmentation_color = fz._buffers["rgb"].clone()
    rec = fz.coarsen(2)
    want, inc = ref.coarsen(fine, BOX_A[0], 2, kind)
    origin, vs, off, nvox = coarse_lattice(GRID.origin, GRID.voxel_size, BOX_A[0], BOX_A[1], 2)
    assert (rec.factor, rec.old_index_offset, rec.old_nvox, rec.index_offset, rec.nvox) == (2,) + BOX_A + (off, nvox) == (2,) + BOX_A + _box(fz)
    assert rec.voxel_size == vs == fz.voxel_size == 2 * GRID.voxel_size and rec.old_voxel_size == GRID.voxel_size
    assert torch.equal(rec.origin, origin) and torch.equal(fz.origin, origin) and torch.equal(rec.old_origin, GRID.origin)
    assert fz._feat_stale and fz._workspace is None and fz._buffers["fuse_stats"].data_ptr() == stats_ptr and fz.clip is clip
    assert not hasattr(fz, "voxel_obj_idx") and not hasattr(fz, "objects_segmentation_color")
    assert rec.rows_blended.is_cuda and rec.rows_blended.dtype == torch.int64 and rec.rows_blended.dim() == 0
    assert (int(rec.rows_blended), int(rec.rows_copied), int(rec.tsdf_blended), int(rec.tsdf_copied)) == inc and min(inc) > 0
    # the volume as it stands (the clear still owed): the small fields, and the rows of the voxels that have one
    raw = _grids(_raw(fz, seem), nvox, kind)
    for name in _names(seem):
        rows = name in ("clip_feat", "labels_one_hot")
        keep = want["weight"] > 0 if rows else np.ones(nvox, bool)
        assert np.array_equal(_np_bits(raw[name])[keep], _np_bits(want[name])[keep]), f"{name} differs from the restatement"
    fresh = _load(_module_at(scan, origin, vs, (off, nvox), seem, fdt), want)
    for name in ("axis_x", "axis_y", "axis_z", "xyz_world"):
        assert torch.equal(_bits(fz._buffers[name]), _bits(fresh._buffers[name])), name
    _fuse(fz, fr[m:n], seem)
    _fuse(fresh, fr[m:n], seem)
    return fz, fresh, rec, want


def _assert_same_volume(fz, fresh, seem, before):
    touched = 0
    for name in _names(seem):
        got, want = getattr(fz, name), getattr(fresh, name)
        if name in ("weight", "tsdf_weight", "labels_one_hot"):
            assert torch.equal(got, want), f"{name}: counts differ from the fresh module's"
        else:  # values, bit for bit but for the sign of a zero
            assert torch.equal(got, want), f"{name} differs from the fresh module's"
        if name == "weight":
            touched = int((got.cpu() != torch.from_numpy(before["weight"]).reshape(-1)).sum())
    assert touched > 50, "the later frames touched next to nothing: the test means nothing"


@pytest.mark.parametrize("seem", [pytest.param(True, id="ClipSeemFusion"), pytest.param(False, id="ClipFusion")])
def test_fusion_goes_on_after_coarsening_per_frame_pipeline(seem):
    from spatially_aware_ai_amd.clip_seem_fusion import discover_objects
    from spatially_aware_ai_amd.objects import describe_objects

    dim = 64
    fz, fresh, rec, before = _fused_then_coarsened(dim, 6, 11, seem)
    assert fresh.stats()["window_rows"] == 0, "not the per-frame pipeline"
    _assert_same_volume(fz, fresh, seem, before)
    # ---- the module's other calls, against the same calls on the fresh module
    fr = _scan(dim, 11).frames
    pose, k = fr[0]["pose"][0].cuda(), fr[0]["K"][0].cuda()
    va, vb = fz.render(pose, k, H, W), fresh.render(pose, k, H, W)
    assert int(va.hit.sum()) > 0 and int(va.voxel.max()) < fz.weight.numel()
    for name in ("depth", "voxel", "rgb", "hit") + (("label",) if seem else ()):
        assert torch.equal(getattr(va, name), getattr(vb, name)), f"render: {name}"
    text = torch.randn(3, dim, generator=torch.Generator().manual_seed(3)).cuda()
    qa, qb = fz.render_query(text, pose, k, H, W), fresh.render_query(text, pose, k, H, W)
    assert torch.equal(qa.relevance, qb.relevance) and bool(torch.isfinite(qa.relevance[qa.hit]).all())
    if seem:
        names, colors = syn.scene_class_names(), syn.scene_class_colors()
        grid_a, grid_b = fz.label_index().view(*rec.nvox), fresh.label_index().view(*rec.nvox)
        assert torch.equal(grid_a, grid_b) and int((grid_a >= 0).sum()) > 50
        know_a, obj_a = discover_objects(grid_a, names, colors, arrays=True)
        know_b, obj_b = discover_objects(grid_b, names, colors, arrays=True)
        assert torch.equal(obj_a, obj_b) and len(know_a["unique_objects"]) >= 1
        da, db = describe_objects(fz, obj_a, know_a), describe_objects(fresh, obj_b, know_b)
        assert da.ids == db.ids and torch.equal(da.feat, db.feat) and np.array_equal(da.centroid_world, db.centroid_world)
        assert np.array_equal(da.extent_world, db.extent_world) and np.array_equal(da.count, db.count)
        for m, obj in ((fz, obj_a), (fresh, obj_b)):  # (what ClipSeemFusion.extract_mesh samples beside colour and features)
            m.voxel_obj_idx = obj
            m.objects_segmentation_color = m.rgb.clone()
    ma, mb = fz.extract_mesh(), fresh.extract_mesh()
    assert len(ma[1]) > 20 and np.array_equal(ma[0], mb[0]) and np.array_equal(ma[1], mb[1])
    for got, want in zip(ma[2:], mb[2:]):
        assert np.array_equal(np.asarray(torch.as_tensor(got).cpu()), np.asarray(torch.as_tensor(want).cpu())), "extract_mesh: a vertex attribute"


def test_fusion_goes_on_after_coarsening_frame_ordered_windows(rows_form):
    fz, fresh, rec, before = _fused_then_coarsened(256, 24, 40, True)
    assert fresh.stats()["window_rows"] > 0 and fz.stats()["window_rows"] > fresh.stats()["window_rows"], "the windowed path did not run"
    _assert_same_volume(fz, fresh, True, before)


@pytest.mark.parametrize("fdt", [pytest.param(torch.float32, id="f32"), pytest.param(torch.bfloat16, id="bf16"),
                                 pytest.param(torch.float16, id="fp16")])
def test_volumes_of_two_voxel_sizes_are_joined_by_coarsening_the_finer_one(fdt):
    dim, m, n = 64, 6, 11
    kind = KIND_OF[fdt]
    scan = _scan(dim, n)
    fr = scan.frames
    box_b = ((-3, 2, -5), (30, 24, 33))
    origin, vs, off_b, n_b = coarse_lattice(GRID.origin, GRID.voxel_size, box_b[0], box_b[1], 2)
    box_a = ((-1, 0, -1), (14, 12, 16))  # a box of the coarse lattice that holds part of B's and more
    a = _fuse(_module_at(scan, origin, vs, box_a, True, fdt), fr[:m])
    b = _fuse(_module(scan, box_b, True, fdt), fr[m:n])
    a_before = _grids(_snapshot(a), box_a[1], kind)
    b_fine = _grids(_snapshot(b), box_b[1], kind)
    with pytest.raises(SafError, match="not on the same lattice"):
        a.absorb(b)
    rec = b.coarsen(2)
    assert (rec.index_offset, rec.nvox) == (off_b, n_b) and torch.equal(torch.as_tensor(b.origin), torch.as_tensor(a.origin))
    out = a.absorb(b, grow=False)
    b_coarse, _ = ref.coarsen(b_fine, box_b[0], 2, kind)
    off = tuple(s - o for s, o in zip(box_a[0], off_b))
    want, inc = aref.absorb(b_coarse, a_before, off, kind)
    assert inc == (int(out.rows_blended), int(out.rows_copied), int(out.tsdf_blended), int(out.tsdf_copied)) and inc[0] > 10 and inc[1] > 0
    got = _grids(_snapshot(a), box_a[1], kind)
    for name in NAMES:
        assert np.array_equal(_np_bits(got[name]), _np_bits(want[name])), f"{name} differs from the two restatements"


# ---- (g) stale rows, queued frames ---------------------------------------------------------------------------------------------
def test_coarsen_of_a_volume_whose_rows_are_still_stale(rows_form):
    dim = 256
    scan = _scan(dim, 64)
    mine = scan.frames[16:40]  # (24 frames: the windowed path)
    twin = _fuse(_module(scan, BOX_A), mine)
    twin.coarsen(2)
    want = _snapshot(twin)
    assert int((want["weight"] > 0).sum()) > 200
    fz = _stale(scan, BOX_A, mine)
    rec = fz.coarsen(2)
    assert fz._feat_stale, "the clear is no longer owed"
    assert not bool(torch.isnan(fz._buffers["clip_feat"][fz._buffers["weight"] > 0]).any()), "a stale row reached a coarse voxel"
    assert int(rec.rows_blended) > 0 and int(rec.rows_copied) > 0
    for name in NAMES:
        assert torch.equal(_bits(getattr(fz, name)), _bits(want[name])), f"{name} differs from the coarsening of a cleared twin"
    assert int(_bits(fz.clip_feat)[fz.weight == 0].abs().max()) == 0, "a row of an untouched voxel does not read as zero"
    assert int(fz.labels_one_hot[fz.weight == 0].abs().max()) == 0


def test_coarsen_behind_the_queue_of_one_frame_calls(rows_form):
    dim, m = 256, 40
    scan = _scan(dim, 64)
    fr = scan.frames
    fz = _module(scan, BOX_A, defer=True)
    _one_by_one(fz, fr[:m])
    q = fz.__dict__["_queue"]
    assert fz.pending_frames + q.ring.sess_frames == m and fz.pending_frames > 0 and fz._queue_busy(), "the calls did not go through the queue"
    rec = fz.coarsen(2)
    assert fz.__dict__["_queue"] is q and not fz._queue_busy() and fz.pending_frames == 0 and fz.clip.calls == m
    fz2 = _module(scan, BOX_A, defer=True)
    _one_by_one(fz2, fr[:m])
    fz2.flush()
    torch.cuda.synchronize()
    rec2 = fz2.coarsen(2)
    assert int(rec.rows_blended) == int(rec2.rows_blended) > 0 and int(rec.rows_copied) == int(rec2.rows_copied) > 0
    for name in NAMES:
        assert torch.equal(_bits(getattr(fz, name)), _bits(getattr(fz2, name))), f"{name} differs from the flushed case"
    # the module afterwards: the queue takes frames again, at the coarse size
    _one_by_one(fz, fr[m:m + 4])
    assert fz.pending_frames > 0, "the calls after the coarsening did not go through the queue"
    view = fz.render(fr[0]["pose"][0].cuda(), fr[0]["K"][0].cuda(), H, W)
    assert int(view.hit.sum()) > 0 and fz.pending_frames == 0 and fz.stats()["frames"] == m + 4


# ---- (h) the scene flow ---------------------------------------------------------------------------------------------------------
def test_coarsen_scene_runs_the_later_stages_on_the_coarse_volume(rows_form, tmp_path):
    from spatially_aware_ai_amd.clip_seem_fusion import discover_objects
    from spatially_aware_ai_amd.scene import coarsen_scene, reconstruct_scene
    from test_scene_extend_gpu import DIM, N_OLD, _Part
    from test_scene_extend_gpu import H as SH
    from test_scene_extend_gpu import W as SW

    scan = syn.SyntheticScan(23, N_OLD, SW, SH, DIM)
    names, colors = syn.scene_class_names(), syn.scene_class_colors()
    clip, seg = syn.ReplayClip(scan, class_names=names), syn.ReplaySeg(scan)
    config = {"voxel_size": 0.08, "trunc_vox": 3, "clip_patch_size": scan.patch, "clip_patch_stride": scan.stride}
    first = reconstruct_scene(_Part(scan, 0, N_OLD), config, clip, seg, names, colors)
    assert clip.calls == N_OLD == 32 and seg.calls == N_OLD
    fz = first.fusion
    fine_box = _box(fz)
    fine = _grids({name: getattr(fz, name).clone() for name in NAMES}, fine_box[1], "f32")
    origin, vs, off, nvox = coarse_lattice(fz.origin, fz.voxel_size, fine_box[0], fine_box[1], 2)
    res = coarsen_scene(first, 2, names, colors, out_dir=str(tmp_path))
    assert clip.calls == N_OLD and seg.calls == N_OLD, "a frame went through the backbones again"
    assert res.fusion is fz and res.scene_knowledge["scan_version"] == 1 and res.object_matches is None
    for k in ("coarsen", "label_argmax", "objects", "extract_mesh", "object_meshes"):
        assert res.seconds[k] > 0, k
    assert _box(fz) == (off, nvox) and torch.equal(torch.as_tensor(res.nvox), fz.nvox) and torch.equal(torch.as_tensor(res.origin), origin)
    assert float(fz.voxel_size) == 0.16 == res.scene_knowledge["voxel_size"] and res.scene_knowledge["nvox"] == list(nvox)
    assert res.scene_knowledge["index_offset"] == list(off) and res.xyz is first.xyz
    saved = json.load(open(res.paths["scene_knowledge"]))
    assert saved["voxel_size"] == 0.16 and saved["nvox"] == list(nvox) and saved["scan_version"] == 1
    # ---- the volume is the restatement's
    want, _ = ref.coarsen(fine, fine_box[0], 2)
    got = _grids({name: getattr(fz, name) for name in NAMES}, nvox, "f32")
    for name in NAMES:
        assert np.array_equal(_np_bits(got[name]), _np_bits(want[name])), f"{name} differs from the restatement"
    # ---- the stages behind the fusion, run again on that volume
    grid = fz.label_index().view(*nvox)
    assert torch.equal(res.onehot_to_index, grid) and int((grid >= 0).sum()) > 50
    knowledge, obj = discover_objects(grid, names, colors, arrays=True)
    assert torch.equal(res.voxel_obj_idx, obj) and torch.equal(fz.voxel_obj_idx, obj)
    assert list(res.scene_knowledge["unique_objects"]) == list(knowledge["unique_objects"]) and len(knowledge["unique_objects"]) >= 1
    verts, faces = fz.extract_mesh()[:2]
    assert np.array_equal(res.verts, verts) and np.array_equal(res.faces, faces) and len(faces) > 50
