"""The object layer: what the scan knows about each discovered object as a whole, and text queries answered per object.

The reference's server is object-centred -- ``/merge_objects``, ``/rename_object``, ``/memorize_objects`` (app_unity.py), the
per-object ``{"clip_feats", "rgb", "voxels"}`` that ``flood_fill_3d`` hands the in-situ classifier (handy_utils.py:400-404),
``merge_objects`` and ``mark_object_of_interest`` (handy_utils.py:501-582).  Here:

  * ``object_slots``      -- ``voxel_obj_idx`` + ``scene_knowledge`` -> a dense object number per voxel;
  * ``object_stats``      -- saf_object_stats (include/saf.h): one segmented reduction over the volume on the HIP device --
                             count, box, coordinate sum, fused members, weight sum, mean colour, mean normalised feature row;
  * ``describe_objects``  -- the same for a fusion module and its scene knowledge: an ``ObjectDescriptors``;
  * ``ObjectDescriptors.query`` -- the existing text-query scan over the K descriptor rows: "which object is the mug, where is
                             it, how big is it" without a heat map over 16.8 M voxels;
  * ``merge_objects`` / ``mark_object_of_interest`` -- the reference's bookkeeping, optionally relabelling the grid;
  * ``object_overlap``    -- saf_object_overlap: the voxels every object of one labelling shares with every object of another
                             labelling of the same lattice, on the HIP device;
  * ``assign_identities`` / ``match_objects`` / ``carry_identities`` -- which object of a scan's new version is which object
                             of the previous one (kept in place, moved, absorbed into a user's merge, new, missing), and the
                             scene knowledge and index grid under the previous identities.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _abi
from ._lib import SafError, check, current_stream_ptr, lib, require_cuda
from .clip_seem_fusion import _obj_counts
from .clipfusion import _query_scan

_NORMALIZE = {"l2": _abi.SAF_NORM_L2, "clamp": _abi.SAF_NORM_L2_CLAMP, "clamp_min": _abi.SAF_NORM_L2_CLAMP,
              _abi.SAF_NORM_L2: _abi.SAF_NORM_L2, _abi.SAF_NORM_L2_CLAMP: _abi.SAF_NORM_L2_CLAMP}


def object_slots(voxel_obj_idx, scene_knowledge):
    """``(slot int32 [N] on the device, ids list[str])``: object ``ids[k]`` owns the voxels whose ``voxel_obj_idx`` equals its
    ``object_index`` (slot k there); every other voxel gets -1.  Objects with ``removed`` set are left out; two objects that
    share an ``object_index`` are an error.  (Index plumbing in torch, on whatever device ``voxel_obj_idx`` lives.)"""
    ids, index = [], []
    for oid, obj in scene_knowledge["unique_objects"].items():
        if obj.get("removed"):
            continue
        ids.append(oid)
        index.append(int(obj["object_index"]))
    if len(set(index)) != len(index):
        dup = sorted(i for i in set(index) if index.count(i) > 1)
        raise ValueError(f"objects share an object_index: {dup}")
    flat = voxel_obj_idx.reshape(-1)
    if not ids:
        return torch.full_like(flat, -1, dtype=torch.int32), ids
    vals, perm = torch.sort(torch.tensor(index, dtype=torch.int64, device=flat.device))
    f = flat.long()
    pos = torch.searchsorted(vals, f).clamp_(max=len(ids) - 1)
    slot = torch.where(vals[pos] == f, perm[pos], torch.full_like(pos, -1))
    return slot.to(torch.int32), ids


def object_stats(weight, rgb, clip_feat, nvox, slot, n_objects, normalize="l2", want=("n_fused", "weight_sum", "coord_sum", "rgb", "feat")):
    """saf_object_stats on a volume's buffers (``weight`` [N] i32, ``rgb`` [N,3] f32, ``clip_feat`` [N,D] f32 / bf16; contiguous,
    on the HIP device) and ``slot`` [N] i32: a dict of device tensors -- ``count`` [K] i64 and ``bbox`` [K,6] i32 always, the
    names in ``want`` besides (outputs not wanted are passed as NULL; without "feat" no feature row is read)."""
    for t, name in ((weight, "weight"), (clip_feat, "clip_feat"), (slot, "slot")):
        require_cuda(t, name)
    mode = _NORMALIZE.get(normalize)
    if mode is None:
        raise ValueError(f"normalize must be 'l2' or 'clamp', not {normalize!r} (raw rows cannot be summed exactly)")
    nx, ny, nz = (int(v) for v in nvox)
    n, k = nx * ny * nz, int(n_objects)
    dev = weight.device
    d = int(clip_feat.shape[1])
    if slot.dtype != torch.int32 or slot.numel() != n or weight.numel() != n or clip_feat.shape[0] != n:
        raise ValueError("slot must be int32 [N], weight [N] and clip_feat [N,D] for N = nx ny nz")
    for t, name in ((weight, "weight"), (rgb, "rgb"), (clip_feat, "clip_feat"), (slot, "slot")):
        if t is not None and not t.is_contiguous():
            raise SafError(f"{name} must be contiguous")
    if rgb is None and "rgb" in want:
        raise ValueError("the mean colour needs the volume's rgb buffer")
    ft = {torch.float32: _abi.SAF_F32, torch.bfloat16: _abi.SAF_BF16}.get(clip_feat.dtype)
    if ft is None:
        raise SafError("object descriptors take f32 and bf16 volumes")
    p = _abi.ptr
    vol = _abi.SafVolume(nx, ny, nz, d, 0, ft, _abi.SAF_RUNNING_MEAN, 0.0, None, None, None, None, None, p(weight), p(rgb),
                         p(clip_feat), None)
    return _object_stats(vol, dev, slot, k, d, mode, want)


def _object_stats(vol, dev, slot, k, d, mode, want):
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    out = {"count": e(k, torch.int64), "bbox": e((k, 6), torch.int32)}
    shapes = {"n_fused": (k, torch.int64), "weight_sum": (k, torch.int64), "coord_sum": ((k, 3), torch.int64),
              "rgb": ((k, 3), torch.float32), "feat": ((k, d), torch.float32)}
    for name in want:
        out[name] = e(*shapes[name])
    L = lib()
    n = vol.nx * vol.ny * vol.nz
    wsb = L.saf_object_stats_workspace_bytes(n, k, d)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
    p = _abi.ptr
    with torch.cuda.device(dev):
        rc = L.saf_object_stats(C.byref(vol), p(slot), k, mode, p(out["count"]), p(out.get("n_fused")), p(out.get("weight_sum")),
                                p(out["bbox"]), p(out.get("coord_sum")), p(out.get("rgb")), p(out.get("feat")), p(ws), wsb,
                                current_stream_ptr())
    check(rc, "saf_object_stats")
    return out


@dataclass
class ObjectQueryResult:
    """What ``ObjectDescriptors.query`` returns."""

    ids: list
    relevance: torch.Tensor  # [K, L] f32 on the device
    order: np.ndarray        # object numbers by descending relevance of the LAST label; of equal values the smaller first
    descriptors: "ObjectDescriptors"

    def best(self, n=1):
        """The ``n`` most relevant objects: ``(id, relevance, centroid_world [3], (bbox_min [3], bbox_max [3]))`` each."""
        d = self.descriptors
        last = self.relevance[:, -1].cpu().numpy() if len(self.ids) else np.zeros(0, np.float32)
        return [(self.ids[k], float(last[k]), d.centroid_world[k], (d.bbox_min[k], d.bbox_max[k])) for k in self.order[:int(n)]]

    def paint(self, slot):
        """The last label's relevance per voxel ([N] f32 on the device), 0 where the voxel has no object: one gather."""
        k = len(self.ids)
        if k == 0:
            return torch.zeros(slot.shape, dtype=torch.float32, device=slot.device)
        s = slot.long()
        inside = (s >= 0) & (s < k)
        return torch.where(inside, self.relevance[:, -1][s.clamp(0, k - 1)], torch.zeros((), device=slot.device))


@dataclass
class ObjectDescriptors:
    """One row per object of a scan (``describe_objects``).  The small per-object arrays live on the host (NumPy), ``feat`` on
    the device.  Boxes are in voxel indices of the module's grid; ``centroid_world`` = origin + voxel_size (coord_sum / count)
    and ``extent_world`` = voxel_size (bbox_max - bbox_min + 1) in fp64 (NaN / 0 for an object without voxels)."""

    ids: list
    object_index: np.ndarray   # [K] i64
    count: np.ndarray          # [K] i64 voxels
    n_fused: np.ndarray        # [K] i64 voxels with weight > 0: what rgb and feat average over
    weight_sum: np.ndarray     # [K] i64
    bbox_min: np.ndarray       # [K,3] i32
    bbox_max: np.ndarray       # [K,3] i32
    coord_sum: np.ndarray      # [K,3] i64
    centroid_world: np.ndarray  # [K,3] f64
    extent_world: np.ndarray   # [K,3] f64
    rgb: np.ndarray            # [K,3] f32
    feat: torch.Tensor         # [K,D] f32 on the device: mean of the members' normalised rows
    origin: np.ndarray = field(default_factory=lambda: np.zeros(3))
    voxel_size: float = 1.0
    nvox: tuple = (0, 0, 0)
    index_offset: tuple = (0, 0, 0)  # the grid's first voxel on the module's lattice (``origin`` already includes it)

    def __len__(self):
        return len(self.ids)

    @staticmethod
    def _world(origin, voxel_size, count, coord_sum, bbox_min, bbox_max):
        cnt = count.astype(np.float64)[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            centroid = origin[None, :] + voxel_size * (coord_sum.astype(np.float64) / cnt)
        extent = voxel_size * np.maximum(bbox_max.astype(np.float64) - bbox_min.astype(np.float64) + 1.0, 0.0)
        return centroid, extent

    def query(self, text_features, epilogue="softmax", scale=100.0):
        """The text query of ``Clip.run_query`` per object: ``query_scan`` (saf_query_scan, SAF_NORM_L2) over ``feat`` against
        ``text_features`` [L, >= D]; epilogue "softmax" or "scores".  Returns an ``ObjectQueryResult``."""
        epi = {"scores": _abi.SAF_Q_SCORES, "softmax": _abi.SAF_Q_SOFTMAX}.get(epilogue)
        if epi is None:
            raise ValueError(f"query takes the epilogues 'scores' and 'softmax', not {epilogue!r}")
        text_features = torch.as_tensor(text_features)
        if len(self.ids) == 0:
            rel = torch.zeros((0, text_features.shape[0]), dtype=torch.float32, device=self.feat.device)
            return ObjectQueryResult(self.ids, rel, np.zeros(0, np.int64), self)
        rel = _query_scan(self.feat, text_features, epi, scale=scale, normalize=_abi.SAF_NORM_L2)
        order = torch.sort(rel[:, -1], descending=True, stable=True).indices.cpu().numpy()
        return ObjectQueryResult(self.ids, rel, order, self)

    def merged(self, ids, new_id, object_index=None):
        """The descriptors after the objects ``ids`` have become one object ``new_id`` (last row; the others keep their order):
        counts, fused counts, weight sums, coordinate sums and boxes combine exactly; the mean colour and feature row are the
        ``n_fused``-weighted means of the parts' rows in fp64, rounded once to f32 -- within two f32 roundings of what
        ``describe_objects`` computes from the relabelled grid (the parts' rows were rounded once themselves)."""
        pos = [self.ids.index(i) for i in ids]
        if not pos or len(set(pos)) != len(pos):
            raise ValueError("merged() needs one or more distinct object ids")
        keep = [k for k in range(len(self.ids)) if k not in set(pos)]
        nf = self.n_fused[pos]
        tot = int(nf.sum())
        w = nf.astype(np.float64) / tot if tot > 0 else np.zeros(len(pos))
        rgb = (self.rgb[pos].astype(np.float64) * w[:, None]).sum(0).astype(np.float32)
        wd = torch.from_numpy(w).to(self.feat.device)
        feat = (self.feat[pos].double() * wd[:, None]).sum(0).float()

        def cat(a, new):
            return np.concatenate([a[keep], np.asarray(new, dtype=a.dtype)[None]], axis=0)

        count, coord = cat(self.count, self.count[pos].sum()), cat(self.coord_sum, self.coord_sum[pos].sum(0))
        bmin, bmax = cat(self.bbox_min, self.bbox_min[pos].min(0)), cat(self.bbox_max, self.bbox_max[pos].max(0))
        centroid, extent = self._world(self.origin, self.voxel_size, count, coord, bmin, bmax)
        return ObjectDescriptors(
            ids=[self.ids[k] for k in keep] + [new_id],
            object_index=cat(self.object_index, self.object_index[pos[0]] if object_index is None else object_index),
            count=count, n_fused=cat(self.n_fused, tot), weight_sum=cat(self.weight_sum, self.weight_sum[pos].sum()),
            bbox_min=bmin, bbox_max=bmax, coord_sum=coord, centroid_world=centroid, extent_world=extent,
            rgb=np.concatenate([self.rgb[keep], rgb[None]], axis=0),
            feat=torch.cat([self.feat[keep], feat[None]], dim=0), origin=self.origin, voxel_size=self.voxel_size, nvox=self.nvox,
            index_offset=self.index_offset)


def describe_objects(fusion, voxel_obj_idx, scene_knowledge, normalize="l2"):
    """``ObjectDescriptors`` of the objects of ``scene_knowledge`` (``discover_objects``) over the volume of ``fusion`` (a
    ``ClipFusion`` / ``ClipSeemFusion`` holding the whole grid; frames still queued behind ``integrate()`` are fused first):
    one saf_object_stats call.  ``normalize``: "l2" (f / |f|, NaN -> 0, what the text query applies) or "clamp"
    (f / max(|f|, 0.1), the eval scripts')."""
    mode = _NORMALIZE.get(normalize)
    if mode is None:
        raise ValueError(f"normalize must be 'l2' or 'clamp', not {normalize!r} (raw rows cannot be summed exactly)")
    if getattr(fusion, "_shard_stripes", None) is not None or fusion.x_planes is not None:
        raise SafError("describe_objects() needs the whole grid: this module holds a slab / the stripes of a voxel-sharded volume")
    vol = fusion._c_volume()  # (joins the queue: the volume holds every frame handed to integrate())
    dev = fusion._buffers["weight"].device
    nvox = tuple(int(v) for v in fusion.nvox)
    voxel_obj_idx = torch.as_tensor(voxel_obj_idx).to(dev)
    if voxel_obj_idx.numel() != nvox[0] * nvox[1] * nvox[2]:
        raise ValueError(f"voxel_obj_idx has {voxel_obj_idx.numel()} entries, the grid {nvox} voxels")
    slot, ids = object_slots(voxel_obj_idx, scene_knowledge)
    k, d = len(ids), int(fusion.n_clip_feats)
    uo = scene_knowledge["unique_objects"]
    index = np.array([int(uo[i]["object_index"]) for i in ids], dtype=np.int64)
    origin = np.asarray(torch.as_tensor(fusion.origin).detach().cpu().numpy(), dtype=np.float64).reshape(3)
    voxel_size = float(fusion.voxel_size)
    index_offset = tuple(int(v) for v in fusion.index_offset)
    origin = origin + voxel_size * np.asarray(index_offset, dtype=np.float64)
    if k == 0:
        z = lambda shape, dt: np.zeros(shape, dtype=dt)
        return ObjectDescriptors(ids, index, z(0, np.int64), z(0, np.int64), z(0, np.int64), z((0, 3), np.int32), z((0, 3), np.int32),
                                 z((0, 3), np.int64), z((0, 3), np.float64), z((0, 3), np.float64), z((0, 3), np.float32),
                                 torch.zeros((0, d), dtype=torch.float32, device=dev), origin, voxel_size, nvox, index_offset)
    out = _object_stats(vol, dev, slot, k, d, mode, ("n_fused", "weight_sum", "coord_sum", "rgb", "feat"))
    h = {name: out[name].cpu().numpy() for name in ("count", "n_fused", "weight_sum", "bbox", "coord_sum", "rgb")}
    bmin, bmax = h["bbox"][:, :3].copy(), h["bbox"][:, 3:].copy()
    centroid, extent = ObjectDescriptors._world(origin, voxel_size, h["count"], h["coord_sum"], bmin, bmax)
    return ObjectDescriptors(ids, index, h["count"], h["n_fused"], h["weight_sum"], bmin, bmax, h["coord_sum"], centroid, extent,
                             h["rgb"], out["feat"], origin, voxel_size, nvox, index_offset)


def mark_object_of_interest(scene_knowledge, insitu_model, object_list):
    """handy_utils.py:501-523: the listed objects become ``user_modified`` with their own id as ``gt_label``, and the ids join
    ``insitu_model.labels`` (the classifier's training labels)."""
    if len(object_list) < 1:
        return scene_knowledge
    unique_objects = scene_knowledge["unique_objects"]
    for obj_id in object_list:
        if obj_id not in unique_objects:  # (the reference prints "object ... not found")
            continue
        unique_objects[obj_id]["user_modified"] = True
        if obj_id not in insitu_model.labels:
            insitu_model.labels.append(obj_id)
        unique_objects[obj_id]["gt_label"] = obj_id
    return scene_knowledge


def _join_voxels(a, b):
    from .io import ArrayList

    if isinstance(a, ArrayList) or isinstance(b, ArrayList):
        return ArrayList(np.concatenate([np.asarray(a).reshape(-1, 3), np.asarray(b).reshape(-1, 3)], axis=0), tuples=True)
    a += b  # in place, as the reference does on its shallow copy
    return a


def merge_objects(scene_knowledge, vertex_obj_idx, insitu_model, merge_list, new_label, voxel_obj_idx=None):
    """handy_utils.py:526-582 (``/merge_objects`` with several ids, ``/rename_object`` with one): the objects of ``merge_list``
    become ONE object -- a copy of the first with the others' voxels appended -- under the id ``"<label>:<running count>"``
    (``"-merged"`` is appended to the label of a real merge; a label that already carries ``:n`` counts under its stem), which
    joins ``insitu_model.labels``; its ``object_index`` is that label's index.  Returns ``(new_id, scene_knowledge)`` -- or
    ``scene_knowledge`` alone for an empty list, as the reference does.  ``vertex_obj_idx`` is accepted and left alone (the
    reference's update of it is commented out).

    ``voxel_obj_idx`` (not in the reference, where the step is commented out): a device grid whose voxels of the merged objects
    are relabelled in place to the new ``object_index``, so that ``describe_objects`` sees the merge."""
    if len(merge_list) < 1:
        return scene_knowledge
    if len(merge_list) > 1 and "merged" not in new_label:
        new_label = f"{new_label}-merged"
    unique_objects = scene_knowledge["unique_objects"]
    object_counts = scene_knowledge["object_counts"]
    new_label, class_label = _obj_counts(object_counts, new_label)
    if new_label not in insitu_model.labels:
        insitu_model.labels.append(new_label)
    obj_index = insitu_model.labels.index(new_label)
    target_object = unique_objects[merge_list[0]].copy()
    old_index = [int(unique_objects[obj_id]["object_index"]) for obj_id in merge_list]
    target_object["merged"] = len(merge_list) > 1
    target_object["user_modified"] = True
    target_object["gt_label"] = new_label
    target_object["class_label"] = class_label
    target_object["object_index"] = obj_index
    for i, obj_id in enumerate(merge_list):
        if i > 0:
            target_object["voxels"] = _join_voxels(target_object["voxels"], unique_objects[obj_id]["voxels"])
        del unique_objects[obj_id]
    unique_objects[new_label] = target_object
    scene_knowledge["unique_objects"] = unique_objects
    if voxel_obj_idx is not None:
        old = torch.tensor(old_index, dtype=voxel_obj_idx.dtype, device=voxel_obj_idx.device)
        voxel_obj_idx.masked_fill_(torch.isin(voxel_obj_idx, old), obj_index)
    return new_label, scene_knowledge


# --------------------------------------------------------------------------------- identities across scan versions
def object_overlap(slot_a, nvox_a, slot_b, nvox_b, offset, n_a, n_b):
    """saf_object_overlap (include/saf.h) on two slot grids of one lattice (``object_slots``; int32, contiguous, on the HIP
    device): voxel (x, y, z) of ``b`` is voxel (x, y, z) + ``offset`` of ``a``, ``offset`` = b's index offset - a's.  A dict of
    device tensors: ``pair`` [n_a, n_b] i64 shared voxels, ``in_a`` [n_a] / ``in_b`` [n_b] i64 members inside the overlap."""
    for t, name in ((slot_a, "slot_a"), (slot_b, "slot_b")):
        require_cuda(t, name)
        if not t.is_contiguous():
            raise SafError(f"{name} must be contiguous")
    na3, nb3 = tuple(int(v) for v in nvox_a), tuple(int(v) for v in nvox_b)
    off = tuple(int(v) for v in offset)
    n_a, n_b = int(n_a), int(n_b)
    if slot_a.dtype != torch.int32 or slot_b.dtype != torch.int32 or slot_a.numel() != na3[0] * na3[1] * na3[2] or \
            slot_b.numel() != nb3[0] * nb3[1] * nb3[2]:
        raise ValueError("slot_a and slot_b must be int32 with nx ny nz entries of their grids")
    if slot_a.device != slot_b.device:
        raise ValueError("slot_a and slot_b live on different devices")
    dev = slot_a.device
    out = {"pair": torch.empty((max(n_a, 0), max(n_b, 0)), dtype=torch.int64, device=dev),
           "in_a": torch.empty(max(n_a, 0), dtype=torch.int64, device=dev), "in_b": torch.empty(max(n_b, 0), dtype=torch.int64, device=dev)}
    L = lib()
    wsb = L.saf_object_overlap_workspace_bytes(n_a, n_b)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
    p = _abi.ptr
    with torch.cuda.device(dev):
        rc = L.saf_object_overlap(p(slot_a), *na3, p(slot_b), *nb3, *off, n_a, n_b, p(out["pair"]), p(out["in_a"]), p(out["in_b"]),
                                  p(ws), wsb, current_stream_ptr())
    check(rc, "saf_object_overlap")
    return out


KIND_NEW, KIND_KEPT, KIND_ABSORBED, KIND_MOVED = 0, 1, 2, 3


def _take_one_to_one(score, a_idx, b_idx, free_a, free_b, match_of_b, kind_of_b, kind):
    """Greedy one-to-one matching of the candidates (a_idx[i], b_idx[i]) by descending score, then a, then b."""
    for i in np.lexsort((b_idx, a_idx, -score)):
        a, b = int(a_idx[i]), int(b_idx[i])
        if free_a[a] and free_b[b]:
            free_a[a] = free_b[b] = False
            match_of_b[b], kind_of_b[b] = a, kind


def assign_identities(pair, in_a, in_b, count_a, count_b, class_a, class_b, merged_a, cos, iou_min=0.25, contain_min=0.5,
                      cos_min=0.9, size_ratio_min=0.5):
    """Which new object ``b`` is which previous object ``a`` (host arrays, NumPy; nothing is launched): ``(match_of_b [n_b] i64,
    kind_of_b [n_b] i64)`` -- an index into ``a`` or -1, and 0 new / 1 kept / 2 absorbed / 3 moved.  ``pair``, ``in_a``, ``in_b``
    are ``object_overlap``'s counts, ``count_*`` the full member counts, ``class_*`` class ids, ``merged_a`` the previous objects'
    ``merged`` flag, ``cos`` [n_a, n_b] the cosine of the two versions' descriptor rows.  Comparisons in fp64; ties go to the
    smaller ``a``, then the smaller ``b``.  The four knobs are policy, not tolerances.

    1. absorb (merged ``a`` only: a user's merge is not undone by the next scan): every ``b`` with a merged ``a`` such that
       ``pair > 0`` and ``pair >= contain_min in_b`` goes to the ``a`` with the largest ``pair``; an ``a`` that absorbed takes no
       part below.
    2. in place: free pairs with ``pair > 0`` and ``pair >= iou_min (in_a + in_b - pair)``, by descending ``pair / union``,
       greedily, one to one.  Class is not compared: a chair that version 2 calls a couch is still the same object.
    3. moved: free ``a`` and ``b`` of one class with ``cos >= cos_min`` and ``min(count) >= size_ratio_min max(count)``, by
       descending ``cos``, greedily, one to one.
    Unmatched ``b`` are new; an ``a`` that no ``b`` names is missing."""
    pair = np.asarray(pair, dtype=np.int64)
    n_a, n_b = pair.shape
    pf = pair.astype(np.float64)
    in_a, in_b = np.asarray(in_a, dtype=np.float64).reshape(n_a), np.asarray(in_b, dtype=np.float64).reshape(n_b)
    count_a, count_b = np.asarray(count_a, dtype=np.float64).reshape(n_a), np.asarray(count_b, dtype=np.float64).reshape(n_b)
    class_a, class_b = np.asarray(class_a).reshape(n_a), np.asarray(class_b).reshape(n_b)
    merged_a = np.asarray(merged_a, dtype=bool).reshape(n_a)
    cos = np.asarray(cos, dtype=np.float64).reshape(n_a, n_b)
    match_of_b, kind_of_b = np.full(n_b, -1, dtype=np.int64), np.zeros(n_b, dtype=np.int64)
    free_a, free_b = np.ones(n_a, dtype=bool), np.ones(n_b, dtype=bool)
    # 1. absorb
    ok = merged_a[:, None] & (pair > 0) & (pf >= float(contain_min) * in_b[None, :])
    if ok.any():
        best = np.where(ok, pair, -1).argmax(axis=0)  # (argmax takes the first, i.e. smallest, a among equal counts)
        for b in np.nonzero(ok.any(axis=0))[0]:
            match_of_b[b], kind_of_b[b] = best[b], KIND_ABSORBED
            free_b[b] = False
        free_a[np.unique(match_of_b[kind_of_b == KIND_ABSORBED])] = False
    # 2. in place
    union = in_a[:, None] + in_b[None, :] - pf
    ok = free_a[:, None] & free_b[None, :] & (pair > 0) & (pf >= float(iou_min) * union)
    a_idx, b_idx = np.nonzero(ok)
    _take_one_to_one(pf[a_idx, b_idx] / union[a_idx, b_idx], a_idx, b_idx, free_a, free_b, match_of_b, kind_of_b, KIND_KEPT)
    # 3. moved
    lo, hi = np.minimum(count_a[:, None], count_b[None, :]), np.maximum(count_a[:, None], count_b[None, :])
    ok = free_a[:, None] & free_b[None, :] & (class_a[:, None] == class_b[None, :]) & (cos >= float(cos_min)) & \
        (lo >= float(size_ratio_min) * hi)
    a_idx, b_idx = np.nonzero(ok)
    _take_one_to_one(cos[a_idx, b_idx], a_idx, b_idx, free_a, free_b, match_of_b, kind_of_b, KIND_MOVED)
    return match_of_b, kind_of_b


@dataclass
class ObjectMatches:
    """What ``match_objects`` decides: ids of the previous and of the new version's scene knowledge."""

    kept: list = field(default_factory=list)           # [(prev_id, new_id, iou)]
    absorbed: list = field(default_factory=list)       # [(prev_id, [new_ids])]: parts of a user's merge
    moved: list = field(default_factory=list)          # [(prev_id, new_id, cos, displacement_world [3] f64)]
    new: list = field(default_factory=list)            # [new_id]
    missing: list = field(default_factory=list)        # [prev_id]
    class_changed: list = field(default_factory=list)  # [prev_id] of kept objects whose class_id differs in the new version


def match_objects(prev, new, overlap, knowledge_prev, knowledge_new, **knobs):
    """``ObjectMatches`` of two versions of a scan: ``prev`` / ``new`` are their ``ObjectDescriptors`` (``describe_objects``),
    ``overlap`` is ``object_overlap`` of their slot grids (None when either version has no object), ``knowledge_*`` supply each
    object's ``class_id`` and the previous objects' ``merged`` flag; ``knobs`` are ``assign_identities``'s.  The cosine of the
    descriptor rows is formed on the device (rows normalised, a row of zeros gives 0); the rule runs on the host.  A moved
    object's ``displacement_world`` is new centroid - old centroid, formed on the lattice: voxel_size times the difference of the
    two mean voxel indices, each counted from the lattice's voxel 0, in fp64."""
    n_a, n_b = len(prev), len(new)
    uo_a, uo_b = knowledge_prev["unique_objects"], knowledge_new["unique_objects"]
    out = ObjectMatches()
    if n_a == 0 or n_b == 0:
        out.new, out.missing = list(new.ids), list(prev.ids)
        return out
    fa = torch.nan_to_num(prev.feat / prev.feat.norm(dim=1, keepdim=True), nan=0.0, posinf=0.0, neginf=0.0)
    fb = torch.nan_to_num(new.feat.to(fa.device) / new.feat.to(fa.device).norm(dim=1, keepdim=True), nan=0.0, posinf=0.0, neginf=0.0)
    cos = (fa @ fb.T).double().cpu().numpy()
    pair, in_a, in_b = (overlap[k].cpu().numpy() for k in ("pair", "in_a", "in_b"))
    class_a = np.array([int(uo_a[i]["class_id"]) for i in prev.ids], dtype=np.int64)
    class_b = np.array([int(uo_b[i]["class_id"]) for i in new.ids], dtype=np.int64)
    merged_a = np.array([bool(uo_a[i].get("merged")) for i in prev.ids], dtype=bool)
    match_of_b, kind_of_b = assign_identities(pair, in_a, in_b, prev.count, new.count, class_a, class_b, merged_a, cos, **knobs)
    parts = {}
    for b in range(n_b):
        a, kind = int(match_of_b[b]), int(kind_of_b[b])
        if kind == KIND_KEPT:
            union = int(in_a[a]) + int(in_b[b]) - int(pair[a, b])
            out.kept.append((prev.ids[a], new.ids[b], float(pair[a, b]) / float(union)))
            if class_a[a] != class_b[b]:
                out.class_changed.append(prev.ids[a])
        elif kind == KIND_ABSORBED:
            parts.setdefault(a, []).append(new.ids[b])
        elif kind == KIND_MOVED:
            where = lambda d, k: d.coord_sum[k].astype(np.float64) / float(d.count[k]) + np.asarray(d.index_offset, dtype=np.float64)
            out.moved.append((prev.ids[a], new.ids[b], float(cos[a, b]), float(new.voxel_size) * (where(new, b) - where(prev, a))))
        else:
            out.new.append(new.ids[b])
    out.absorbed = [(prev.ids[a], parts[a]) for a in sorted(parts)]
    named = set(int(a) for a in match_of_b if a >= 0)
    out.missing = [prev.ids[a] for a in range(n_a) if a not in named]
    return out


def carry_identities(knowledge_prev, knowledge_new, voxel_obj_idx_new, matches):
    """The bookkeeping that makes ``matches`` visible: ``(scene_knowledge, voxel_obj_idx)`` of the new version under the previous
    version's identities.  Neither input dict nor ``voxel_obj_idx_new`` is changed.  The new objects are walked in
    ``knowledge_new``'s order (discovery order):

    * kept / moved: the entry is keyed by the PREVIOUS id and carries the previous ``object_index``, ``gt_label``,
      ``user_modified`` and ``merged``; ``voxels`` (and ``mesh``) are the new entry's.  A ``user_modified`` object keeps its
      ``class_label`` and ``color`` too; otherwise ``class_id``, ``class_label`` and ``color`` follow the new labelling.
    * absorbed: one entry under the previous id with the previous labels; the parts' ``voxels`` joined in discovery order.
    * new: the id counts on from a copy of the PREVIOUS ``object_counts`` (an id is never used again, not even a missing
      object's); ``object_index`` counts down from below ``min(-1, every previous object_index)``.
    ``voxel_obj_idx`` is relabelled through a lookup table on its device: every object's index marks exactly its ``voxels``.
    ``unchanged_objects`` = kept + absorbed, ``moved_objects`` (entries gain ``displacement_world``), ``new_objects``, and
    ``missing_objects`` = the previous entries of the missing objects (as flood_fill_3d fills it from ``scene_knowledge_prev``)."""
    uo_prev, uo_new = knowledge_prev["unique_objects"], knowledge_new["unique_objects"]
    role = {}
    for prev_id, new_id, _ in matches.kept:
        role[new_id] = ("kept", prev_id, None)
    for prev_id, new_id, _, disp in matches.moved:
        role[new_id] = ("moved", prev_id, disp)
    for prev_id, new_ids in matches.absorbed:
        for new_id in new_ids:
            role[new_id] = ("absorbed", prev_id, None)
    counts = dict(knowledge_prev.get("object_counts", {}))
    next_index = min([-1] + [int(o["object_index"]) for o in uo_prev.values()]) - 1
    unique, unchanged, moved, fresh = {}, {}, {}, {}
    old_index, final_index = [], []
    for new_id, entry in uo_new.items():
        kind, prev_id, disp = role.get(new_id, ("new", None, None))
        if kind == "new":
            obj = dict(entry)
            oid, class_label = _obj_counts(counts, entry["class_label"])
            obj.update(class_label=class_label, gt_label=oid, object_index=next_index)
            next_index -= 1
            unique[oid] = fresh[oid] = obj
        elif kind == "absorbed":
            obj = unique.get(prev_id)
            if obj is None:
                obj = dict(uo_prev[prev_id])
                obj.pop("mesh", None)
                vox = entry["voxels"]
                obj["voxels"] = list(vox) if isinstance(vox, list) else vox  # (_join_voxels appends to a list in place)
                unique[prev_id] = unchanged[prev_id] = obj
            else:
                obj["voxels"] = _join_voxels(obj["voxels"], entry["voxels"])
        else:
            old = uo_prev[prev_id]
            obj = dict(entry)
            for key in ("object_index", "gt_label", "user_modified", "merged"):
                obj[key] = old[key]
            if old.get("user_modified"):
                obj["class_label"], obj["color"] = old["class_label"], old.get("color")
            if kind == "moved":
                obj["displacement_world"] = [float(v) for v in disp]
                moved[prev_id] = obj
            else:
                unchanged[prev_id] = obj
            unique[prev_id] = obj
        old_index.append(int(entry["object_index"]))
        final_index.append(int(obj["object_index"]))
    grid = torch.as_tensor(voxel_obj_idx_new)
    if old_index:
        vals, perm = torch.sort(torch.tensor(old_index, dtype=torch.int64, device=grid.device))
        to = torch.tensor(final_index, dtype=torch.int64, device=grid.device)[perm]
        f = grid.reshape(-1).long()
        pos = torch.searchsorted(vals, f).clamp_(max=len(old_index) - 1)
        grid = torch.where(vals[pos] == f, to[pos], f).to(grid.dtype).view(grid.shape)
    else:
        grid = grid.clone()
    knowledge = dict(knowledge_new)
    knowledge.update(unique_objects=unique, object_counts=counts, unchanged_objects=unchanged, moved_objects=moved, new_objects=fresh,
                     missing_objects={i: uo_prev[i] for i in matches.missing})
    return knowledge, grid
