"""The ScanNet open-vocabulary segmentation eval (reference eval_scannet_segmentation.py) on the device.

The reference scores a fused scan in three steps, each a HIP kernel here:

* ``segment`` (:546-561): clamp-normalised vertex features against the prompts' text embeddings, ``softmax(100 F T^T)``,
  a full argsort of which the eval reads columns ``[:, :5]`` and ``[:, 0]`` -- here the top k labels per vertex and their
  probabilities (``saf_query_topk``);
* the label transfer (:585-587): a KD-tree nearest neighbour from every GT mesh vertex to the predicted mesh's vertices --
  here an exact grid search (``saf_nearest_points``);
* the scoring (:589-601, :655-659): top-1 / top-5 correct counts per class and sklearn's confusion matrix
  (``saf_segmentation_counts``); IoU, mIoU and mAcc from them on the host (:722-732).

The class lists (ScanNet20 / ScanNet200 labels, prompts, colours) are the caller's: pass them in.
"""
from __future__ import annotations

import glob
import json
import os

import numpy as np
import torch

from . import _abi
from ._lib import check, current_stream_ptr, lib
from .io import load_ply_vertices

__all__ = [
    "segment",
    "topk_labels",
    "nearest_vertices",
    "transfer_labels",
    "get_gt_labels",
    "segmentation_counts",
    "eval_scene",
    "summarize",
    "evaluate",
]

_FEAT_DTYPES = {torch.float32: _abi.SAF_F32, torch.bfloat16: _abi.SAF_BF16, torch.float16: _abi.SAF_F16}


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _workspace(nbytes):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=_device())


def topk_labels(feats, text, k=5, scale=100.0, normalize=_abi.SAF_NORM_L2_CLAMP):
    """Per row of ``feats`` [N, D] (f32, bf16 or f16 on the device) the ``k`` labels of largest ``scale * <f^, t_l>``, best
    first (equal scores: the smaller label), and their softmax probabilities over all labels of ``text`` [L, D]:
    ``(labels int64 [N, k], probs f32 [N, k])``.  ``f^`` is the row under ``normalize`` (a ``saf_query_normalize``)."""
    if feats.dtype not in _FEAT_DTYPES:
        raise ValueError(f"feature dtype {feats.dtype}: f32, bf16 or f16")
    if feats.dim() != 2 or text.dim() != 2 or text.shape[1] != feats.shape[1]:
        raise ValueError(f"features {tuple(feats.shape)} and text {tuple(text.shape)} do not match")
    n, d = feats.shape
    nl = text.shape[0]
    if not 1 <= k <= min(8, nl):
        raise ValueError(f"k = {k}: 1 <= k <= min(8, {nl} labels)")
    if feats.stride(1) != 1:
        feats = feats.contiguous()
    text = text.to(device=feats.device, dtype=torch.float32).contiguous()
    index = torch.empty((n, k), dtype=torch.int32, device=feats.device)
    prob = torch.empty((n, k), dtype=torch.float32, device=feats.device)
    ws = _workspace(lib().saf_query_topk_workspace_bytes(n, nl, k))
    rc = lib().saf_query_topk(feats.data_ptr(), _FEAT_DTYPES[feats.dtype], n, feats.stride(0), d, text.data_ptr(), nl, text.stride(0),
                              float(scale), int(normalize), int(k), index.data_ptr(), prob.data_ptr(), ws.data_ptr(), ws.numel(),
                              current_stream_ptr())
    check(rc, "saf_query_topk")
    return index.long(), prob


def _vertex_features(vertex_feats):
    if isinstance(vertex_feats, (str, os.PathLike)):
        vertex_feats = np.load(vertex_feats)
    t = torch.as_tensor(vertex_feats)
    if t.dtype not in _FEAT_DTYPES:
        t = t.float()
    t = t.to(_device())
    if t.dim() != 2:
        raise ValueError(f"vertex features of shape {tuple(t.shape)}: [V, D] expected")
    # the reference normalises, then raises on NaN (:549-554): a NaN or an infinity in the input is where it does
    if not bool(torch.isfinite(t).all()):
        raise ValueError("found nans")
    return t


def segment(clip, vertex_feats, prompts, k=5):
    """``segment`` of eval_scannet_segmentation.py:546-561: ``vertex_feats`` (a ``.npy`` path, an array or a tensor [V, D])
    clamp-normalised, against ``clip.text_inference(prompts)``, ``softmax(100 F T^T)``.  Returns ``(labels int64 [V, k],
    probs f32 [V, k])`` on the device: the first k columns of the reference's argsort and the matching ``relevance``."""
    feats = _vertex_features(vertex_feats)
    text = torch.as_tensor(clip.text_inference(prompts))
    return topk_labels(feats, text, k=k, scale=100.0, normalize=_abi.SAF_NORM_L2_CLAMP)


def _points(p, what):
    t = torch.as_tensor(p)
    t = t.to(device=_device(), dtype=torch.float32).reshape(-1, 3).contiguous()
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"{what}: non-finite coordinates")
    return t


def nearest_vertices(ref, query):
    """For every point of ``query`` [M, 3] the nearest point of ``ref`` [N, 3] (scipy.spatial.KDTree(ref).query(query),
    eval_scannet_segmentation.py:585-586): ``(index int64 [M], dist2 f64 [M])``, exact -- squared distances in fp64, of
    equal distances the smaller index.  The coordinates are taken as fp32: fp64 input is rounded to fp32 first."""
    r, q = _points(ref, "ref"), _points(query, "query")
    if r.shape[0] == 0:
        raise ValueError("nearest_vertices: no reference points")
    m = q.shape[0]
    index = torch.empty(m, dtype=torch.int32, device=r.device)
    dist2 = torch.empty(m, dtype=torch.float64, device=r.device)
    if m:
        ws = _workspace(lib().saf_nearest_workspace_bytes(r.shape[0], m))
        rc = lib().saf_nearest_points(r.data_ptr(), r.shape[0], q.data_ptr(), m, index.data_ptr(), dist2.data_ptr(), ws.data_ptr(),
                                      ws.numel(), current_stream_ptr())
        check(rc, "saf_nearest_points")
    return index.long(), dist2


def transfer_labels(pred_vertices, gt_vertices, pred_labels):
    """``pred_labels[nn]`` with nn the nearest predicted vertex of every GT vertex (eval_scannet_segmentation.py:585-587)."""
    idx, _ = nearest_vertices(pred_vertices, gt_vertices)
    return torch.as_tensor(pred_labels).to(idx.device)[idx]


def get_gt_labels(scan_dir, labels):
    """``get_gt_labels`` of eval_scannet_segmentation.py:493-543 with the class list ``labels`` passed in: per vertex of the
    scan's ``_vh_clean_2`` mesh the index of its category in ``labels``, -1 where the vertex's segment has no annotation or
    its category is not in the list.  A ``"sofa"`` category raises, as in the reference.  Returns int32 [V]."""
    scan = os.path.basename(os.path.normpath(scan_dir))
    with open(os.path.join(scan_dir, f"{scan}.aggregation.json")) as f:
        agg = json.load(f)
    with open(os.path.join(scan_dir, f"{scan}_vh_clean_2.0.010000.segs.json")) as f:
        segs = json.load(f)
    segments = {}
    for group in agg["segGroups"]:
        for seg in group["segments"]:
            segments[seg] = group["label"]
    seg_idx = np.asarray(segs["segIndices"], dtype=np.int64)
    if seg_idx.size == 0:
        return np.full((0,), -1, dtype=np.int32)
    class_to_idx = {c: i for i, c in enumerate(labels)}
    uniq, inv = np.unique(seg_idx, return_inverse=True)
    lut = np.full(len(uniq), -1, dtype=np.int32)
    for j, seg in enumerate(uniq.tolist()):
        if seg in segments:
            category = segments[seg]
            if category == "sofa":
                raise ValueError("gah. is this an alias for couch?")
            lut[j] = class_to_idx.get(category, -1)
    return lut[inv.reshape(-1)]


def segmentation_counts(gt, transferred, n_classes, topk=5, into=None):
    """The reference's scoring counts (eval_scannet_segmentation.py:589-601 and sklearn's ``confusion_matrix(gt, pred[:, 0],
    labels=range(L))``) on the device: ``gt`` [M] class per vertex (outside [0, n_classes): skipped), ``transferred`` [M, k]
    labels best first.  Returns ``into`` -- a dict of int64 device tensors ``cmat`` [L, L], ``ncorrect_top1``,
    ``ncorrect_topk``, ``ntotal`` [L] -- with this call's counts added, or a fresh one."""
    dev = _device()
    g = torch.as_tensor(gt).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    p = torch.as_tensor(transferred).to(device=dev, dtype=torch.int32)
    if p.dim() == 1:
        p = p[:, None]
    p = p.contiguous()
    if p.shape[0] != g.shape[0]:
        raise ValueError(f"{g.shape[0]} GT labels and {p.shape[0]} predictions")
    topk = max(1, min(int(topk), p.shape[1]))
    accumulate = into is not None
    if into is None:
        z = lambda *s: torch.empty(s, dtype=torch.int64, device=dev)
        into = {"cmat": z(n_classes, n_classes), "ncorrect_top1": z(n_classes), "ncorrect_topk": z(n_classes), "ntotal": z(n_classes)}
    rc = lib().saf_segmentation_counts(g.data_ptr(), p.data_ptr(), g.shape[0], p.shape[1], topk, int(n_classes), into["cmat"].data_ptr(),
                                       into["ncorrect_top1"].data_ptr(), into["ncorrect_topk"].data_ptr(), into["ntotal"].data_ptr(),
                                       1 if accumulate else 0, current_stream_ptr())
    check(rc, "saf_segmentation_counts")
    return into


def eval_scene(pred_dir, gt_dir, labels, prompts, clip, k=5):
    """``eval_scene`` of eval_scannet_segmentation.py:564-661 without its four visualisation meshes: reads
    ``vertex_clip_feats.npy`` and ``mesh_rgb.ply`` of ``pred_dir`` and the GT mesh ``<scan>_vh_clean_2.ply`` of ``gt_dir``,
    saves ``gt_vertex_labels.npy`` and ``transferred_vertex_labels.npy`` into ``pred_dir``, and returns ``(cmat int64 [L, L],
    ncorrect_top1, ncorrect_top5, ntotal)`` (int64 [L] each).  ``transferred_vertex_labels.npy`` holds the first ``k``
    labels per GT vertex, [M, k] -- the reference saves the whole [M, L] argsort, of which it reads only these."""
    pred_v = load_ply_vertices(os.path.join(pred_dir, "mesh_rgb.ply"))
    gt_v = load_ply_vertices(os.path.join(gt_dir, f"{os.path.basename(os.path.normpath(gt_dir))}_vh_clean_2.ply"))
    pred_labels, _ = segment(clip, os.path.join(pred_dir, "vertex_clip_feats.npy"), prompts, k=k)
    gt_labels = get_gt_labels(gt_dir, labels)
    transferred = transfer_labels(pred_v, gt_v, pred_labels)
    c = segmentation_counts(torch.from_numpy(gt_labels), transferred, len(labels), topk=5)
    np.save(os.path.join(pred_dir, "transferred_vertex_labels.npy"), transferred.cpu().numpy())
    np.save(os.path.join(pred_dir, "gt_vertex_labels.npy"), gt_labels)
    host = {n: t.cpu().numpy() for n, t in c.items()}
    return host["cmat"], host["ncorrect_top1"], host["ncorrect_topk"], host["ntotal"]


def _nanmean(x):
    x = x[~np.isnan(x)]
    return float(x.mean()) if x.size else float("nan")


def summarize(cmat, ncorrect_top1, ncorrect_topk, ntotal):
    """IoU per class, mIoU, mAcc top-1 and top-k as eval_scannet_segmentation.py:722-732 computes them: ``tp / (tp + fp + fn)``
    from the confusion matrix, ``ncorrect / ntotal`` per class, means over the classes that are not NaN (a class that never
    occurs is NaN and left out, without a warning)."""
    host = lambda a: a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    cmat = host(cmat).astype(np.int64)
    tp = np.diagonal(cmat)
    fn = cmat.sum(axis=-1) - tp
    fp = cmat.sum(axis=0) - tp
    n1, nk, nt = (host(a).astype(np.int64) for a in (ncorrect_top1, ncorrect_topk, ntotal))
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = tp / (tp + fp + fn)
        acc1 = n1 / nt
        acck = nk / nt
    return {"iou": iou, "miou": _nanmean(iou), "macc_top1": _nanmean(acc1), "macc_topk": _nanmean(acck)}


def evaluate(pred_root, gt_root, labels, prompts, clip_factory, scan_name=None):
    """The reference's ``__main__`` loop (eval_scannet_segmentation.py:673-748): every ``scene*`` directory of ``pred_root``
    against the GT directory of the same name under ``gt_root``, with ``clip_factory(pred_dir)`` as that scene's text
    encoder (the reference builds ``Clip`` from the scene's config.yml).  Writes ``scene_cmats.json`` and
    ``global_cmat.npy`` into ``pred_root`` and returns ``summarize`` of the summed counts."""
    pred_dirs = [d for d in sorted(glob.glob(os.path.join(pred_root, "scene*"))) if os.path.isdir(d)]
    gt_dirs = {os.path.basename(d): d for d in sorted(glob.glob(os.path.join(gt_root, "scene*")))}
    if scan_name is not None:
        pred_dirs = [d for d in pred_dirs if os.path.basename(d) == scan_name]
        if not pred_dirs:
            raise ValueError(f"couldn't find a scan called {scan_name}")
    n = len(labels)
    total = [np.zeros((n, n), np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)]
    scene_cmats = {}
    for pred_dir in pred_dirs:
        name = os.path.basename(pred_dir)
        if name not in gt_dirs:
            raise ValueError(f"couldn't find gt_dir for scene: {name}")
        out = eval_scene(pred_dir, gt_dirs[name], labels, prompts, clip_factory(pred_dir))
        scene_cmats[name] = out[0].tolist()
        for acc, part in zip(total, out):
            acc += part
    with open(os.path.join(pred_root, "scene_cmats.json"), "w") as f:
        json.dump(scene_cmats, f)
    np.save(os.path.join(pred_root, "global_cmat.npy"), total[0])
    return summarize(*total)
