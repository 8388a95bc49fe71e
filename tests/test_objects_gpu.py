"""GPU: saf_object_stats and the object layer (spatially_aware_ai_amd/objects.py) against an fp64 torch restatement of the contract
in include/saf.h.

Bars (none of them taken from the device's output):
  * count, n_fused, weight_sum, bbox, coord_sum: equal.
  * feat_mean: |got - want| <= 2^-20 mean_n |f^_n,c| + 2^-30 per element.  Per term the kernel computes the row's sum of squares in
    fp32 (8 terms per lane in sequence, 6 butterfly levels: at most 15 roundings, half of which survive the square root), one sqrtf,
    one IEEE division; the mean is rounded once to f32: about 9.5 x 2^-24 relative in all, 0.6 x 2^-20.  The second term is the
    2^-31 quantisation of rint(v 2^30) with a factor of two.
  * rgb_mean: <= 2^-24 + 2^-30 (the clamp is exact; quantisation 2^-31 per term; one rounding of a value <= 1).
  * merged(): the parts' rows were rounded to f32 once each, the merged row is rounded once, and so is the recomputed one:
    3 x 2^-24 of sum_i w_i |m_i|; asserted at 4 x 2^-24 = 2^-22 because the recomputed row's own magnitude is only bounded by
    that sum up to its rounding.
"""
import functools

import numpy as np
import pytest
import torch

from spatially_aware_ai_amd import synthetic as syn

pytestmark = pytest.mark.gpu

GRIDS = {"odd": (33, 30, 41), "pow2": (16, 16, 64)}
FEATS = {"512f32": (512, torch.float32), "512bf16": (512, torch.bfloat16), "64f32": (64, torch.float32), "10f32": (10, torch.float32)}
# rows wider than one 512-column tile: a second grid row of waves that re-reads the row for its norm and flushes features only
WIDE = {"1032f32": (1032, torch.float32), "520bf16": (520, torch.bfloat16), "515f32": (515, torch.float32)}
ALL = ("n_fused", "weight_sum", "coord_sum", "rgb", "feat")


# ------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _volume(grid, feat):
    """weight [N] i32 (a third of them 0), rgb [N,3] f32 (values outside [0, 1] among them), clip_feat [N,D] with zero rows, rows
    under the 0.1 clamp and rows of magnitude 1e4 (planted where tests/test_eval_gpu.py::_feats plants them; the small rows are
    scaled to a norm of about 0.06 at every width, so that the two normalisations differ at every width)."""
    nx, ny, nz = GRIDS[grid]
    d, dtype = {**FEATS, **WIDE}[feat]
    n = nx * ny * nz
    g = torch.Generator().manual_seed(1000 + n + d)
    f = torch.randn(n, d, generator=g)
    f[::97] *= 0.06 / d ** 0.5
    f[5::101] = 0.0
    f[7::89] *= 1e4
    weight = torch.randint(0, 6, (n,), generator=g, dtype=torch.int32)
    weight[torch.rand(n, generator=g) < 0.2] = 0
    rgb = torch.rand(n, 3, generator=g) * 1.4 - 0.2
    return weight.cuda(), rgb.cuda(), f.to(dtype).cuda()


@functools.lru_cache(maxsize=None)
def _slots(grid, k):
    """Runs of random objects along z with every edge the contract names planted on top."""
    nx, ny, nz = GRIDS[grid]
    n = nx * ny * nz
    g = torch.Generator().manual_seed(77 + n + k)
    # random runs of 1..9 voxels in raster order (they cross column ends, as a chunk boundary crosses runs)
    n_runs = n // 2
    lens = torch.randint(1, 10, (n_runs,), generator=g)
    vals = torch.randint(-1, k, (n_runs,), generator=g)  # -1: no object
    slot = torch.repeat_interleave(vals, lens)[:n].to(torch.int32).clone()
    assert slot.numel() == n
    grid3 = slot.view(nx, ny, nz)
    if k >= 7:
        slot[slot == 0] = -1
        slot[slot == 1] = -1
        grid3[nx // 2, ny // 3, nz // 2] = 0            # object 0: one voxel
        #                                                  object 1: no member
        grid3[0, 0, 0] = 2                               # object 2 spans the whole grid
        grid3[nx - 1, ny - 1, nz - 1] = 2
        grid3[3, 4, :] = torch.tensor([3, 4] * nz)[:nz].to(torch.int32)  # two objects alternating voxel by voxel along z
        grid3[3, 5, :] = torch.tensor([4, 3] * nz)[:nz].to(torch.int32)
        grid3[5, 1:4, :] = 5                             # object 5's voxels all get weight 0 below: count > 0, n_fused = 0
        slot[(slot == 5) & (torch.arange(n) // (ny * nz) != 5)] = -1
    else:
        grid3[0, 0, 0] = 0                               # K = 1: the one object spans the whole grid
        grid3[nx - 1, ny - 1, nz - 1] = 0
    # values that mean "no object"
    bad = torch.tensor([-1, -5, k, 2 ** 30], dtype=torch.int32)
    where = torch.randperm(n, generator=g)[:200]
    where = where[(where != 0) & (where != n - 1)]
    keep = slot.clone()
    slot[where] = bad[torch.arange(len(where)) % 4]
    if k >= 7:  # (the planted single voxel stays)
        one = (nx // 2 * ny + ny // 3) * nz + nz // 2
        slot[one] = keep[one]
    return slot.cuda()


def _weight_for(grid, feat, k):
    weight, rgb, f = _volume(grid, feat)
    if k >= 7:
        weight = weight.clone()
        weight[_slots(grid, k) == 5] = 0
    return weight, rgb, f


# ------------------------------------------------------------------------------------------------------------ restatement
def _restate(weight, rgb, feat, nvox, slot, k, normalize):
    nx, ny, nz = nvox
    n = nx * ny * nz
    dev = weight.device
    s = slot.long()
    member = (s >= 0) & (s < k)
    idx = s[member]
    ar = torch.arange(n, device=dev)
    coords = torch.stack((ar // (ny * nz), (ar // nz) % ny, ar % nz), dim=1)
    cm = coords[member]
    out = {"count": torch.bincount(idx, minlength=k)}
    out["coord_sum"] = torch.zeros((k, 3), dtype=torch.int64, device=dev).index_add_(0, idx, cm)
    bmin = torch.tensor([nx, ny, nz], dtype=torch.float64, device=dev).repeat(k, 1)  # (small integers: exact in fp64)
    bmax = torch.full((k, 3), -1.0, dtype=torch.float64, device=dev)
    ix = idx[:, None].expand(-1, 3)
    bmin.scatter_reduce_(0, ix, cm.double(), "amin", include_self=True)
    bmax.scatter_reduce_(0, ix, cm.double(), "amax", include_self=True)
    out["bbox"] = torch.cat((bmin, bmax), dim=1).to(torch.int32)
    fused = member & (weight > 0)
    fi = s[fused]
    nf = torch.bincount(fi, minlength=k)
    out["n_fused"] = nf
    out["weight_sum"] = torch.zeros(k, dtype=torch.int64, device=dev).index_add_(0, fi, weight[fused].long())
    den = nf.double().clamp_min(1.0)[:, None]
    out["rgb"] = torch.zeros((k, 3), dtype=torch.float64, device=dev).index_add_(0, fi, rgb[fused].double().clamp(0.0, 1.0)) / den
    f = feat[fused].double()
    norm = f.norm(dim=1, keepdim=True)
    fh = torch.nan_to_num(f / norm, nan=0.0) if normalize == "l2" else f / norm.clamp_min(0.1)
    d = feat.shape[1]
    out["feat"] = torch.zeros((k, d), dtype=torch.float64, device=dev).index_add_(0, fi, fh) / den
    out["feat_abs"] = torch.zeros((k, d), dtype=torch.float64, device=dev).index_add_(0, fi, fh.abs()) / den
    return out


def _check(got, want, what):
    for name in ("count", "n_fused", "weight_sum", "coord_sum", "bbox"):
        if name in got:
            assert got[name].dtype == (torch.int32 if name == "bbox" else torch.int64)
            assert torch.equal(got[name].long(), want[name].long()), f"{what}: {name}"
    if "rgb" in got:
        err = (got["rgb"].double() - want["rgb"]).abs().max()
        print(f"{what}: rgb_mean max error {float(err):.3g} (allowed {2.0 ** -24 + 2.0 ** -30:.3g})")
        assert float(err) <= 2.0 ** -24 + 2.0 ** -30, f"{what}: rgb_mean"
    if "feat" in got:
        err = (got["feat"].double() - want["feat"]).abs()
        tol = 2.0 ** -20 * want["feat_abs"] + 2.0 ** -30
        print(f"{what}: feat_mean worst error / allowed {float((err / tol).max()):.3g}")
        assert bool((err <= tol).all()), f"{what}: feat_mean off by up to {float((err / tol).max()):.3g} of the bound"
        assert bool((got["feat"][want["n_fused"] == 0] == 0).all())


def _stats(grid, feat, k, normalize, want=ALL):
    from spatially_aware_ai_amd.objects import object_stats

    weight, rgb, f = _weight_for(grid, feat, k)
    return object_stats(weight, rgb, f, GRIDS[grid], _slots(grid, k), k, normalize=normalize, want=want)


# ------------------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("k", [1, 7, 3000])
@pytest.mark.parametrize("feat", list(FEATS))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_object_stats_against_fp64(grid, feat, k):
    weight, rgb, f = _weight_for(grid, feat, k)
    slot = _slots(grid, k)
    if k >= 7:  # the planted edges are what they are meant to be
        cnt = torch.bincount(slot[(slot >= 0) & (slot < k)].long(), minlength=k)
        assert int(cnt[0]) == 1 and int(cnt[1]) == 0 and int(cnt[5]) > 0
    for v in (-1, -5, k, 2 ** 30):
        assert bool((slot == v).any())
    wants = {m: _restate(weight, rgb, f, GRIDS[grid], slot, k, m) for m in ("l2", "clamp")}
    assert not torch.equal(wants["l2"]["feat"], wants["clamp"]["feat"]), "rows under the clamp make the two modes differ"
    for normalize in ("l2", "clamp"):
        want = wants[normalize]
        got = _stats(grid, feat, k, normalize)
        _check(got, want, f"{grid} {feat} K={k} {normalize}")
        if k >= 7:
            nx, ny, nz = GRIDS[grid]
            assert got["bbox"][1].tolist() == [nx, ny, nz, -1, -1, -1] and int(got["count"][1]) == 0
            assert got["bbox"][2].tolist() == [0, 0, 0, nx - 1, ny - 1, nz - 1]
            assert int(got["n_fused"][5]) == 0 and int(got["count"][5]) > 0 and bool((got["rgb"][5] == 0).all())


@pytest.mark.parametrize("feat", list(WIDE))
def test_object_stats_rows_wider_than_a_tile(feat):
    """D = 1032 f32 and 520 bf16 on the vector path, 515 f32 element by element: two and three column tiles."""
    grid, k = "odd", 7
    weight, rgb, f = _weight_for(grid, feat, k)
    slot = _slots(grid, k)
    for normalize in ("l2", "clamp"):
        want = _restate(weight, rgb, f, GRIDS[grid], slot, k, normalize)
        _check(_stats(grid, feat, k, normalize), want, f"{grid} {feat} K={k} {normalize}")


def _bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("feat,k", [("512f32", 7), ("512bf16", 3000), ("10f32", 7), ("1032f32", 7), ("520bf16", 7)])
def test_object_stats_is_reproducible(feat, k):
    a = _stats("odd", feat, k, "l2")
    b = _stats("odd", feat, k, "l2")
    assert set(a) == set(b) == {"count", "bbox", *ALL}
    for name in a:
        assert _bytes_equal(a[name], b[name]), name


def test_object_stats_optional_outputs():
    full = _stats("odd", "64f32", 7, "clamp")
    for want in ((), ("feat",), ("rgb", "n_fused"), ("coord_sum", "weight_sum"), ("n_fused", "weight_sum", "coord_sum", "rgb")):
        part = _stats("odd", "64f32", 7, "clamp", want=want)
        assert set(part) == {"count", "bbox", *want}
        for name in part:
            assert _bytes_equal(part[name], full[name]), (want, name)


def test_object_stats_64_bit_offsets():
    """2^22 voxels x 512 bf16 = 2^31 elements (4 GB of zeros): two small objects in the last x-planes, rows planted there."""
    from spatially_aware_ai_amd.objects import object_stats

    nvox = (64, 256, 256)
    n, d, k = nvox[0] * nvox[1] * nvox[2], 512, 2
    assert n * d == 2 ** 31
    feat = torch.zeros((n, d), dtype=torch.bfloat16, device="cuda")
    weight = torch.zeros(n, dtype=torch.int32, device="cuda")
    rgb = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    slot = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    s3, w3 = slot.view(*nvox), weight.view(*nvox)
    s3[62, 250:253, 100:140] = 0
    s3[63, 255, 251:256] = 1  # the very last rows of the volume
    g = torch.Generator().manual_seed(5)
    for obj in (0, 1):
        rows = torch.nonzero(slot == obj).reshape(-1)
        assert int(rows.max()) * d > 2 ** 31 - 2 ** 26
        feat[rows] = (torch.randn(len(rows), d, generator=g) * 3.0).to(torch.bfloat16).cuda()
        rgb[rows] = torch.rand(len(rows), 3, generator=g).cuda()
        weight[rows] = torch.randint(0, 4, (len(rows),), generator=g, dtype=torch.int32).cuda()
    assert int(slot[n - 1]) == 1
    want = _restate(weight, rgb, feat, nvox, slot, k, "l2")
    got = object_stats(weight, rgb, feat, nvox, slot, k, normalize="l2")
    _check(got, want, "2^31 elements")
    assert got["bbox"].tolist() == [[62, 250, 100, 62, 252, 139], [63, 255, 251, 63, 255, 255]]
    assert int(got["n_fused"].min()) > 0 and float(got["feat"].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------ Python layer
class _Clip:
    feature_dim = 64


class _Model:
    def __init__(self):
        self.labels = ["null", "an earlier label"]
        self.model_trained = False


BOXES = [((1, 2, 3), (4, 6, 9)), ((6, 0, 0), (6, 0, 0)), ((8, 3, 2), (15, 9, 4)), ((8, 3, 10), (9, 17, 23)),
         ((17, 1, 1), (19, 2, 20)), ((0, 10, 12), (5, 16, 13))]  # inclusive corners, disjoint
INDEX = [-2, -3, 3, -4, 7, -5]  # negative (first scan) and positive (re-identified) object indices


@pytest.fixture(scope="module")
def boxes_scene():
    from spatially_aware_ai_amd import ClipSeemFusion

    nvox, vs, d = (20, 18, 24), 0.05, 64
    origin = torch.tensor([-0.3, 0.1, 1.2])
    fz = ClipSeemFusion(origin, vs, torch.tensor(nvox), 3 * vs, False, 10, 10, _Clip(), None, keep_xyz_world=False, device="cuda").cuda()
    g = torch.Generator().manual_seed(3)
    proto = torch.linalg.qr(torch.randn(d, len(BOXES), generator=g)).Q.T.contiguous()  # K orthonormal prototypes
    n = nvox[0] * nvox[1] * nvox[2]
    grid = torch.full(nvox, -1, dtype=torch.int32)
    feat, weight, rgb = torch.zeros(n, d), torch.zeros(n, dtype=torch.int32), torch.zeros(n, 3)
    know = {"unique_objects": {}, "object_counts": {}}
    for k, ((x0, y0, z0), (x1, y1, z1)) in enumerate(BOXES):
        grid[x0:x1 + 1, y0:y1 + 1, z0:z1 + 1] = INDEX[k]
        rows = torch.nonzero(grid.reshape(-1) == INDEX[k]).reshape(-1)
        noise = torch.randn(len(rows), d, generator=g)
        noise = 0.1 * noise / noise.norm(dim=1, keepdim=True)
        feat[rows] = (proto[k][None] + noise) * (0.5 + torch.rand(len(rows), 1, generator=g))
        weight[rows] = torch.randint(1, 4, (len(rows),), generator=g, dtype=torch.int32)
        rgb[rows] = torch.rand(len(rows), 3, generator=g)
        label = f"thing{k % 4}"
        know["object_counts"][label] = know["object_counts"].get(label, 0) + 1
        oid = f"{label}:{know['object_counts'][label]}"
        vox = torch.nonzero(grid == INDEX[k]).tolist()
        know["unique_objects"][oid] = {"class_id": k % 4, "class_label": label, "voxels": [tuple(v) for v in vox],
                                       "object_index": INDEX[k], "gt_label": oid, "user_modified": INDEX[k] > 0, "merged": False,
                                       "removed": False, "color": None}
    fz.clip_feat.copy_(feat.cuda())
    fz.weight.copy_(weight.cuda())
    fz.rgb.copy_(rgb.cuda())
    return dict(fz=fz, grid=grid.cuda(), know=know, proto=proto, nvox=nvox, vs=vs, origin=origin)


def test_describe_objects_boxes(boxes_scene):
    from spatially_aware_ai_amd import _lib
    from spatially_aware_ai_amd.objects import describe_objects

    s = boxes_scene
    d = describe_objects(s["fz"], s["grid"], s["know"])
    assert d.ids == list(s["know"]["unique_objects"]) and d.object_index.tolist() == INDEX and len(d) == len(BOXES)
    lo = np.array([b[0] for b in BOXES], dtype=np.int64)
    hi = np.array([b[1] for b in BOXES], dtype=np.int64)
    assert np.array_equal(d.bbox_min, lo) and np.array_equal(d.bbox_max, hi)
    assert np.array_equal(d.count, (hi - lo + 1).prod(axis=1)) and np.array_equal(d.n_fused, d.count)
    origin = s["origin"].numpy().astype(np.float64)
    assert d.centroid_world.dtype == np.float64 and d.extent_world.dtype == np.float64
    assert np.array_equal(d.centroid_world, origin[None] + s["vs"] * ((lo + hi).astype(np.float64) / 2.0))
    assert np.array_equal(d.extent_world, s["vs"] * (hi - lo + 1).astype(np.float64))
    assert d.feat.is_cuda and d.feat.dtype == torch.float32 and tuple(d.feat.shape) == (len(BOXES), 64)
    # each descriptor points at its prototype
    cos = torch.nn.functional.normalize(d.feat.cpu(), dim=1) @ s["proto"].T
    assert torch.equal(cos.argmax(dim=1), torch.arange(len(BOXES))) and float(cos.diag().min()) > 0.99
    with pytest.raises(ValueError, match="normalize"):
        describe_objects(s["fz"], s["grid"], s["know"], normalize=False)
    # a voxel-sharded module is refused, as render() refuses it
    s["fz"].x_planes = torch.arange(s["nvox"][0])
    try:
        with pytest.raises(_lib.SafError, match="whole grid"):
            describe_objects(s["fz"], s["grid"], s["know"])
    finally:
        s["fz"].x_planes = None


def test_object_query_ranks_and_paints(boxes_scene):
    from spatially_aware_ai_amd.objects import describe_objects, object_slots

    s = boxes_scene
    d = describe_objects(s["fz"], s["grid"], s["know"])
    slot, ids = object_slots(s["grid"], s["know"])
    assert ids == d.ids
    k_obj = len(BOXES)
    # the split scan's stated bound, as tests/test_eval_gpu.py restates it
    CUT, ACC = 4.0 * 2.0 ** -22, 3.0e-7
    fh = torch.nn.functional.normalize(d.feat.double(), dim=1)
    for k in range(k_obj):
        text = torch.cat((s["proto"][:k], s["proto"][k + 1:], s["proto"][k:k + 1]))  # text k last: the column that ranks
        res = d.query(text)
        assert res.ids == d.ids and tuple(res.relevance.shape) == (k_obj, k_obj) and res.relevance.is_cuda
        assert int(res.order[0]) == k and sorted(res.order.tolist()) == list(range(k_obj))
        t = text.double().cuda()
        lg = 100.0 * fh @ t.T
        mag = 100.0 * fh.abs() @ t.abs().T
        p64 = torch.softmax(lg, dim=-1)
        dl = (mag * (CUT + ACC) + 2.0 ** -22 * lg.abs()).max(dim=-1, keepdim=True).values
        assert bool(((res.relevance.double() - p64).abs() <= 1e-6 + 2.0 * p64 * (1.0 - p64) * dl).all())
        last = res.relevance[:, -1]
        assert res.order.tolist() == torch.sort(last, descending=True, stable=True).indices.tolist()
        oid, rel, centroid, (bmin, bmax) = res.best(1)[0]
        assert oid == d.ids[k] and rel == float(last[k]) and np.array_equal(centroid, d.centroid_world[k])
        assert bmin.tolist() == list(BOXES[k][0]) and bmax.tolist() == list(BOXES[k][1])
        assert len(res.best(3)) == 3
        painted = res.paint(slot)
        want = torch.where(slot >= 0, last[slot.clamp_min(0).long()], torch.zeros((), device="cuda"))
        assert painted.dtype == torch.float32 and torch.equal(painted, want) and bool((painted[slot < 0] == 0).all())
    # equal values: the smaller object number first
    tie = d.query(torch.zeros(2, 64), epilogue="scores")
    assert tie.order.tolist() == list(range(k_obj))


def test_merged_equals_recomputation(boxes_scene):
    import copy

    from spatially_aware_ai_amd.objects import describe_objects, merge_objects

    s = boxes_scene
    know, grid, model = copy.deepcopy(s["know"]), s["grid"].clone(), _Model()
    d = describe_objects(s["fz"], grid, know)
    parts = [d.ids[1], d.ids[4], d.ids[2]]
    new_id, know = merge_objects(know, None, model, parts, "desk", voxel_obj_idx=grid)
    index = model.labels.index(new_id)
    assert new_id == "desk-merged:1" and index == 2
    assert int((grid == index).sum()) == int(d.count[[1, 4, 2]].sum()) and not bool(torch.isin(grid, torch.tensor([-3, 7, 3]).cuda()).any())
    m = d.merged(parts, new_id, object_index=index)
    r = describe_objects(s["fz"], grid, know)
    assert m.ids == r.ids == [d.ids[0], d.ids[3], d.ids[5], new_id]
    for name in ("object_index", "count", "n_fused", "weight_sum", "bbox_min", "bbox_max", "coord_sum", "centroid_world", "extent_world"):
        assert np.array_equal(getattr(m, name), getattr(r, name)), name
    assert torch.equal(m.feat[:3], r.feat[:3]) and np.array_equal(m.rgb[:3], r.rgb[:3])
    w = d.n_fused[[1, 4, 2]].astype(np.float64) / d.n_fused[[1, 4, 2]].sum()
    s_feat = (d.feat[[1, 4, 2]].double().abs().cpu().numpy() * w[:, None]).sum(0)
    s_rgb = (np.abs(d.rgb[[1, 4, 2]].astype(np.float64)) * w[:, None]).sum(0)
    assert (np.abs(m.feat[3].double().cpu().numpy() - r.feat[3].double().cpu().numpy()) <= 2.0 ** -22 * s_feat).all()
    assert (np.abs(m.rgb[3].astype(np.float64) - r.rgb[3].astype(np.float64)) <= 2.0 ** -22 * s_rgb).all()


def test_scene_result_object_query():
    """SceneResult.object_query on the small scene of tests/test_scene_pipeline.py."""
    from spatially_aware_ai_amd.scene import reconstruct_scene

    w, h, d, n_frames = 64, 48, 64, 150
    scan = syn.SyntheticScan(11, n_frames, w, h, d)
    names, colors = syn.scene_class_names(), syn.scene_class_colors()
    clip, seg = syn.ReplayClip(scan, class_names=names), syn.ReplaySeg(scan)
    config = {"voxel_size": 0.08, "trunc_vox": 3, "clip_patch_size": scan.patch, "clip_patch_stride": scan.stride}
    res = reconstruct_scene(scan, config, clip, seg, names, colors, object_meshes=False)
    uo = res.scene_knowledge["unique_objects"]
    assert res.objects is None
    out = res.object_query(clip, "chair")
    assert out.ids and set(out.ids) <= set(uo) and len(out.ids) == len(uo)
    labels = sorted(set(o["class_label"] for o in uo.values()) - {"chair"}) + ["chair"]
    assert tuple(out.relevance.shape) == (len(out.ids), len(labels)) and bool(torch.isfinite(out.relevance).all())
    assert res.seconds["object_query"] > 0
    desc = res.objects
    assert desc is not None and np.array_equal(desc.count, [len(uo[i]["voxels"]) for i in out.ids])
    res.object_query(clip, "wall")
    assert res.objects is desc, "the descriptors are computed once"
    # the sphere is one large object of class "chair": it is what the query names first
    oid, rel, centroid, (bmin, bmax) = out.best(1)[0]
    assert uo[oid]["class_label"] == "chair" and 0.0 < rel <= 1.0 and np.isfinite(centroid).all() and (bmax >= bmin).all()
