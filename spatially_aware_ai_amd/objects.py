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
  * ``merge_objects`` / ``mark_object_of_interest`` -- the reference's bookkeeping, optionally relabelling the grid.
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
            feat=torch.cat([self.feat[keep], feat[None]], dim=0), origin=self.origin, voxel_size=self.voxel_size, nvox=self.nvox)


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
    origin = origin + voxel_size * np.asarray(fusion.index_offset, dtype=np.float64)
    if k == 0:
        z = lambda shape, dt: np.zeros(shape, dtype=dt)
        return ObjectDescriptors(ids, index, z(0, np.int64), z(0, np.int64), z(0, np.int64), z((0, 3), np.int32), z((0, 3), np.int32),
                                 z((0, 3), np.int64), z((0, 3), np.float64), z((0, 3), np.float64), z((0, 3), np.float32),
                                 torch.zeros((0, d), dtype=torch.float32, device=dev), origin, voxel_size, nvox)
    out = _object_stats(vol, dev, slot, k, d, mode, ("n_fused", "weight_sum", "coord_sum", "rgb", "feat"))
    h = {name: out[name].cpu().numpy() for name in ("count", "n_fused", "weight_sum", "bbox", "coord_sum", "rgb")}
    bmin, bmax = h["bbox"][:, :3].copy(), h["bbox"][:, 3:].copy()
    centroid, extent = ObjectDescriptors._world(origin, voxel_size, h["count"], h["coord_sum"], bmin, bmax)
    return ObjectDescriptors(ids, index, h["count"], h["n_fused"], h["weight_sum"], bmin, bmax, h["coord_sum"], centroid, extent,
                             h["rgb"], out["feat"], origin, voxel_size, nvox)


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
