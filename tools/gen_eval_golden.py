#!/usr/bin/env python3
"""Generates tests/golden/eval_scene_small.npz: the reference's own ScanNet segmentation eval
(eval_scannet_segmentation.py: ``segment``, ``get_gt_labels``, ``eval_scene`` and the mIoU / mAcc arithmetic of its
``__main__``) run on a small synthetic scene, inputs and outputs stored for tests/test_eval_host.py and
tests/test_eval_gpu.py.

The reference is imported behind stand-in modules (oracle/gen_golden.py's ``import_reference``), with ``open3d``'s mesh
reader answering from the generator's own arrays, its writers doing nothing, and a ``clip`` whose ``text_inference``
returns fixed unit vectors.  The module's ``labels20`` / ``prompts20`` / ``colors20`` are replaced by the generator's
synthetic lists, so no class list of the reference is needed or stored.

The scene has no near-ties: the 1st to 6th logits of every row, and the nearest two predicted vertices of every GT
vertex, are separated by at least 1e-4 relative -- the reference's argsort and KD-tree would otherwise pick an order
that no other implementation is bound to.  The script does nothing when the reference is absent.
Usage:  python tools/gen_eval_golden.py [--out tests/golden]
"""
import argparse
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"

N_PRED, N_GT, D, L, SCAN = 3000, 4000, 64, 20, "scene0000_00"
GAP = 1e-4


def labels_and_prompts():
    labels = [f"thing{i:02d}" for i in range(L - 1)] + ["other"]
    return labels, [f"a photo of a {n}" for n in labels]


def make_scene(seed=20):
    """Inputs of the scene: predicted mesh vertices with features, text embeddings, GT mesh vertices and their JSON."""
    rng = np.random.default_rng(seed)
    text = rng.standard_normal((L, D))
    text /= np.linalg.norm(text, axis=1, keepdims=True)
    text = text.astype(np.float32)
    # predicted vertices on the faces of a room-sized box and a ball inside it; a class per region
    pred = rng.uniform(-1.0, 1.0, (N_PRED, 3))
    face = rng.integers(0, 6, N_PRED)
    pred[np.arange(N_PRED), face // 2] = np.where(face % 2 == 0, -1.0, 1.0)
    ball = rng.random(N_PRED) < 0.25
    b = rng.standard_normal((int(ball.sum()), 3))
    pred[ball] = 0.3 * b / np.linalg.norm(b, axis=1, keepdims=True)
    pred = pred.astype(np.float32)
    rows = np.arange(N_PRED)
    side = (pred[rows, (face // 2 + 1) % 3] > 0).astype(np.int64) + (pred[rows, (face // 2 + 2) % 3] > 0.5)
    region = np.where(ball, L - 1, (face * 3 + side) % (L - 1))

    def logits_ok(f):
        fn = f.astype(np.float64)
        fn = fn / np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 0.1)
        lg = 100.0 * fn @ text.astype(np.float64).T
        s = -np.sort(-lg, axis=1)[:, :6]
        gaps = s[:, :-1] - s[:, 1:]
        rel = np.maximum(np.abs(s[:, :-1]), 1.0)
        return (gaps >= GAP * rel).all(axis=1) & (s[:, 0] - s[:, 5] < 60.0)  # (no softmax value of the six underflows)

    feats = np.zeros((N_PRED, D), np.float32)
    todo = np.ones(N_PRED, bool)
    while todo.any():
        n = int(todo.sum())
        f = 0.5 * text[region[todo]] + 0.12 * rng.standard_normal((n, D))
        mag = rng.choice([1.0, 0.05, 3.0, 1e-3], n, p=[0.7, 0.1, 0.15, 0.05])  # rows under the 0.1 clamp among them
        f = (f * mag[:, None]).astype(np.float32)
        idx = np.flatnonzero(todo)
        ok = logits_ok(f)
        feats[idx[ok]] = f[ok]
        todo[idx[ok]] = False
    # GT vertices: most near the predicted surface, some far from it (outside the box)
    gt = np.empty((N_GT, 3), np.float32)
    near = N_GT - 600
    todo = np.ones(N_GT, bool)
    src = rng.integers(0, N_PRED, N_GT)
    while todo.any():
        n = int(todo.sum())
        idx = np.flatnonzero(todo)
        cand = np.where((idx < near)[:, None], pred[src[idx]] + 0.02 * rng.standard_normal((n, 3)),
                        rng.uniform(-1.0, 1.0, (n, 3)) * 3.0 + np.array([4.0, 0.0, 0.0]))
        cand = cand.astype(np.float32)
        d2 = ((cand.astype(np.float64)[:, None, :] - pred.astype(np.float64)[None]) ** 2).sum(-1)
        two = np.sort(d2, axis=1)[:, :2]
        ok = two[:, 1] - two[:, 0] >= GAP * np.maximum(two[:, 1], 1e-12)
        gt[idx[ok]] = cand[ok]
        todo[idx[ok]] = False
    # ScanNet's annotation files: segments over the GT vertices, groups of segments with a category each
    n_seg = 80
    seg_of = (np.floor((gt[:, 0] + 8) * 2.0) * 7 + np.floor((gt[:, 1] + 8) * 2.0) * 3 + np.floor((gt[:, 2] + 8) * 1.5)).astype(np.int64)
    seg_of = (seg_of % n_seg) * 3 + 5  # sparse segment ids, as ScanNet's are
    labels, _ = labels_and_prompts()
    groups, segs = [], sorted(set(seg_of.tolist()))
    for j, s in enumerate(segs):
        if j % 9 == 4:
            continue  # an unlabelled segment
        cat = labels[j % L] if j % 7 != 3 else f"unlisted{j % 3}"  # categories outside the list
        groups.append({"id": len(groups), "objectId": len(groups), "label": cat, "segments": [s]})
    groups.append({"id": len(groups), "objectId": len(groups), "label": labels[2], "segments": [segs[0]]})  # a later group wins
    agg = {"sceneId": SCAN, "segGroups": groups}
    segjson = {"sceneId": SCAN, "segIndices": seg_of.tolist()}
    colors = rng.uniform(0.1, 1.0, (L, 3)).astype(np.float32)
    return dict(pred_vertices=pred, gt_vertices=gt, feats=feats, text=text, colors=colors,
                aggregation=json.dumps(agg), segs=json.dumps(segjson))


def run_reference(scene):
    sys.path.insert(0, REPO)
    from oracle.gen_golden import import_reference

    import_reference()
    import scipy.spatial  # noqa: F401  (the eval reaches it as scipy.spatial)

    meshes = {}

    class _Mesh:
        def __init__(self, other=None):
            self.vertices = getattr(other, "vertices", None)

    o3d = sys.modules["open3d"]
    o3d.io = types.SimpleNamespace(read_triangle_mesh=lambda p: meshes[os.path.basename(p)], write_triangle_mesh=lambda *a, **k: True)
    o3d.geometry = types.SimpleNamespace(TriangleMesh=_Mesh)
    o3d.utility = types.SimpleNamespace(Vector3dVector=lambda a: a)
    sys.path.insert(0, REF)
    import eval_scannet_segmentation as ev

    labels, prompts = labels_and_prompts()
    ev.labels20, ev.prompts20, ev.colors20 = labels, prompts, scene["colors"]
    text = torch.from_numpy(scene["text"])

    class _Clip:
        def text_inference(self, p):
            assert list(p) == prompts
            return text

    for name, v in (("mesh_rgb.ply", "pred_vertices"), (f"{SCAN}_vh_clean_2.ply", "gt_vertices")):
        m = _Mesh()
        m.vertices = scene[v].astype(np.float64)  # open3d holds float64 vertices
        meshes[name] = m
    with tempfile.TemporaryDirectory() as tmp:
        pred_dir, gt_dir = os.path.join(tmp, "pred", SCAN), os.path.join(tmp, "gt", SCAN)
        os.makedirs(pred_dir)
        os.makedirs(gt_dir)
        np.save(os.path.join(pred_dir, "vertex_clip_feats.npy"), scene["feats"])
        with open(os.path.join(gt_dir, f"{SCAN}.aggregation.json"), "w") as f:
            f.write(scene["aggregation"])
        with open(os.path.join(gt_dir, f"{SCAN}_vh_clean_2.0.010000.segs.json"), "w") as f:
            f.write(scene["segs"])
        pred_labels = ev.segment(_Clip(), os.path.join(pred_dir, "vertex_clip_feats.npy"), prompts)
        gt_labels = ev.get_gt_labels(gt_dir, classes="20")
        _, inds = scipy.spatial.KDTree(meshes["mesh_rgb.ply"].vertices).query(meshes[f"{SCAN}_vh_clean_2.ply"].vertices)
        cmat, n1, n5, nt = ev.eval_scene(pred_dir, gt_dir, "20", _Clip())
    # the __main__ arithmetic over one scene (:722-732)
    tp = np.diagonal(cmat)
    fn = np.sum(cmat, axis=-1) - tp
    fp = np.sum(cmat, axis=0) - tp
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = tp / (tp + fp + fn)
        acc1 = np.array(n1) / np.array(nt)
        acc5 = np.array(n5) / np.array(nt)
        miou, macc1, macc5 = np.nanmean(iou), np.nanmean(acc1), np.nanmean(acc5)
    return dict(pred_top5=pred_labels[:, :5].numpy().astype(np.int64), inds=np.asarray(inds, np.int64),
                gt_labels=np.asarray(gt_labels, np.int32), cmat=np.asarray(cmat, np.int64),
                ncorrect_top1=np.asarray(n1, np.int64), ncorrect_top5=np.asarray(n5, np.int64), ntotal=np.asarray(nt, np.int64),
                iou=iou, miou=np.float64(miou), macc_top1=np.float64(macc1), macc_top5=np.float64(macc5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    if not os.path.isdir(REF):
        print("no reference checkout: nothing generated")
        return
    scene = make_scene()
    out = run_reference(scene)
    labels, prompts = labels_and_prompts()
    path = os.path.join(args.out, "eval_scene_small.npz")
    np.savez_compressed(path, labels=np.array(labels), prompts=np.array(prompts), scan=np.array(SCAN), **scene, **out)
    print("wrote", path, os.path.getsize(path), "bytes; mIoU", out["miou"], "mAcc", out["macc_top1"], out["macc_top5"])


if __name__ == "__main__":
    main()
