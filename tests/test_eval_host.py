"""CPU: the host half of spatially_aware_ai_amd.evaluation -- the PLY vertex reader, get_gt_labels and summarize -- on
hand-built files and against the reference's own results (tests/golden/eval_scene_small.npz, tools/gen_eval_golden.py)."""
import json
import os
import struct

import numpy as np
import pytest

from spatially_aware_ai_amd import evaluation as E
from spatially_aware_ai_amd.io import load_ply_vertices

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_scene_small.npz")


def _verts(n=7, seed=0):
    return np.random.default_rng(seed).standard_normal((n, 3)).astype(np.float32)


def test_ply_binary_little_endian_scannet_layout(tmp_path):
    """ScanNet's _vh_clean_2.ply: float x,y,z; uchar red,green,blue,alpha; then a face list."""
    v = _verts()
    head = ("ply\nformat binary_little_endian 1.0\ncomment VCGLIB generated\nelement vertex 7\nproperty float x\nproperty float y\n"
            "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"
            "element face 2\nproperty list uchar int vertex_indices\nend_header\n")
    body = b"".join(struct.pack("<3f4B", *p, 10, 20, 30, 255) for p in v.tolist())
    body += struct.pack("<B3i", 3, 0, 1, 2) + struct.pack("<B3i", 3, 2, 3, 4)
    p = tmp_path / "scan_vh_clean_2.ply"
    p.write_bytes(head.encode() + body)
    got = load_ply_vertices(p)
    assert got.dtype == np.float32 and np.array_equal(got, v)


def test_ply_binary_big_endian_other_types_and_an_element_before(tmp_path):
    v = _verts(5, 1)
    head = ("ply\nformat binary_big_endian 1.0\nelement camera 2\nproperty list uchar short tag\nproperty double f\n"
            "element vertex 5\nproperty short id\nproperty double x\nproperty double y\nproperty uchar flag\nproperty double z\n"
            "element face 0\nproperty list uchar uint vertex_indices\nend_header\n")
    body = struct.pack(">B2hd", 2, 7, 8, 1.5) + struct.pack(">Bd", 0, 2.5)
    body += b"".join(struct.pack(">hddBd", i, p[0], p[1], 1, p[2]) for i, p in enumerate(v.astype(np.float64).tolist()))
    p = tmp_path / "be.ply"
    p.write_bytes(head.encode() + body)
    assert np.array_equal(load_ply_vertices(p), v)


def test_ply_ascii_with_faces(tmp_path):
    v = _verts(4, 2)
    lines = ["ply", "format ascii 1.0", "comment hand-made", "element vertex 4", "property float x", "property float y",
             "property float z", "property uchar red", "property uchar green", "property uchar blue", "element face 2",
             "property list uchar int vertex_indices", "end_header"]
    lines += [f"{a!r} {b!r} {c!r} 1 2 3" for a, b, c in v.tolist()]
    lines += ["3 0 1 2", "3 1 2 3"]
    p = tmp_path / "a.ply"
    p.write_text("\n".join(lines) + "\n")
    assert np.array_equal(load_ply_vertices(p), v)


def test_ply_rejects_what_is_not_a_mesh(tmp_path):
    p = tmp_path / "x.ply"
    p.write_bytes(b"not a ply\n")
    with pytest.raises(ValueError):
        load_ply_vertices(p)


def _scan_dir(tmp_path, name, seg_indices, groups):
    d = tmp_path / name
    d.mkdir()
    (d / f"{name}.aggregation.json").write_text(json.dumps({"sceneId": name, "segGroups": groups}))
    (d / f"{name}_vh_clean_2.0.010000.segs.json").write_text(json.dumps({"sceneId": name, "segIndices": seg_indices}))
    return str(d)


def test_get_gt_labels_unlabelled_and_unknown_categories(tmp_path):
    labels = ["wall", "floor", "chair"]
    groups = [{"label": "floor", "segments": [4, 9]}, {"label": "lamp", "segments": [2]}, {"label": "chair", "segments": [7]},
              {"label": "wall", "segments": [9]}]  # a later group wins segment 9
    segs = [4, 9, 2, 7, 11, 4, 7, 2, 11, 9]  # 11: no group
    got = E.get_gt_labels(_scan_dir(tmp_path, "scene0001_00", segs, groups), labels)
    assert got.dtype == np.int32
    assert got.tolist() == [1, 0, -1, 2, -1, 1, 2, -1, -1, 0]


def test_get_gt_labels_raises_on_sofa(tmp_path):
    groups = [{"label": "sofa", "segments": [3]}]
    with pytest.raises(ValueError, match="couch"):
        E.get_gt_labels(_scan_dir(tmp_path, "scene0002_00", [1, 3], groups), ["couch"])
    # a sofa segment no vertex uses does not raise (the reference looks at the vertices' segments)
    assert E.get_gt_labels(_scan_dir(tmp_path, "scene0003_00", [1, 2], groups), ["couch"]).tolist() == [-1, -1]


def test_get_gt_labels_equals_the_reference(tmp_path):
    g = np.load(GOLDEN)
    d = tmp_path / str(g["scan"])
    d.mkdir()
    (d / f"{g['scan']}.aggregation.json").write_text(str(g["aggregation"]))
    (d / f"{g['scan']}_vh_clean_2.0.010000.segs.json").write_text(str(g["segs"]))
    got = E.get_gt_labels(str(d), [str(s) for s in g["labels"]])
    assert np.array_equal(got, g["gt_labels"])
    assert (got == -1).any() and (got >= 0).any()


def test_summarize_equals_the_reference():
    g = np.load(GOLDEN)
    s = E.summarize(g["cmat"], g["ncorrect_top1"], g["ncorrect_top5"], g["ntotal"])
    np.testing.assert_allclose(s["iou"], g["iou"], rtol=0, atol=1e-12, equal_nan=True)
    assert abs(s["miou"] - float(g["miou"])) <= 1e-12
    assert abs(s["macc_top1"] - float(g["macc_top1"])) <= 1e-12
    assert abs(s["macc_topk"] - float(g["macc_top5"])) <= 1e-12


def test_summarize_against_numpy_with_absent_classes():
    rng = np.random.default_rng(3)
    c = 12
    cmat = rng.integers(0, 50, (c, c)).astype(np.int64)
    cmat[4, :] = 0
    cmat[:, 4] = 0  # a class that never occurs: NaN, left out
    cmat[7, :] = 0  # a class never in the GT but predicted: IoU 0, accuracy NaN
    nt = cmat.sum(axis=1)
    n1 = np.diagonal(cmat).copy()
    nk = np.minimum(nt, n1 + rng.integers(0, 5, c))
    s = E.summarize(cmat, n1, nk, nt)
    tp = np.diagonal(cmat).astype(np.float64)
    iou = np.array([tp[i] / (cmat[i].sum() + cmat[:, i].sum() - tp[i]) if cmat[i].sum() + cmat[:, i].sum() else np.nan
                    for i in range(c)])
    np.testing.assert_allclose(s["iou"], iou, rtol=1e-15, equal_nan=True)
    assert np.isnan(s["iou"][4]) and s["iou"][7] == 0.0
    ok = ~np.isnan(iou)
    assert abs(s["miou"] - iou[ok].mean()) < 1e-15
    acc = np.array([n1[i] / nt[i] for i in range(c) if nt[i]])
    assert abs(s["macc_top1"] - acc.mean()) < 1e-15
    assert abs(s["macc_topk"] - np.mean([nk[i] / nt[i] for i in range(c) if nt[i]])) < 1e-15
    e = E.summarize(np.zeros((3, 3), np.int64), np.zeros(3), np.zeros(3), np.zeros(3))
    assert np.isnan(e["miou"]) and np.isnan(e["macc_top1"])
