"""GPU: the segmentation eval's kernels (saf_query_topk, saf_nearest_points, saf_segmentation_counts) against fp64 / numpy
restatements, and spatially_aware_ai_amd.evaluation end to end against the reference's own eval_scene (the golden)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from spatially_aware_ai_amd import _abi
from spatially_aware_ai_amd import evaluation as E

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_scene_small.npz")

# the split scan's stated bound (tests/test_split_scan.py, restated): a score is within (CUT + ACC) * sum_k |f_k t_k| of exact
CUT = 4.0 * 2.0 ** -22
ACC = 3.0e-7

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _feats(n, d, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(n, d, generator=g)
    f[::97] *= 0.02        # rows under the 0.1 clamp
    f[5::101] = 0.0        # zero rows
    f[7::89] *= 1e4        # rows of magnitude 1e4
    return f.to(DTYPES[dtype]).cuda()


def _text(nl, d, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(nl, d, generator=g)
    t = t / t.norm(dim=-1, keepdim=True)
    if nl >= 6:
        t[5] = t[2]        # planted exact ties: equal scores, the smaller label first
    if nl >= 71:
        t[70] = t[3]       # ... across two label blocks
    return t.cuda()


def _check_topk(feats, text, k, idx, prob, scale=100.0):
    f = feats.double()
    fh = f / f.norm(dim=-1, keepdim=True).clamp_min(0.1)
    t = text.double()
    lg = scale * fh @ t.T
    mag = scale * fh.abs() @ t.abs().T
    want_v, want_i = torch.sort(lg, dim=-1, descending=True, stable=True)
    want_v, want_i = want_v[:, :k], want_i[:, :k]
    assert idx.shape == want_i.shape and bool((idx >= 0).all()) and bool((idx < text.shape[0]).all())
    got_v = lg.gather(1, idx)
    tol = (mag.gather(1, idx) + mag.gather(1, want_i)) * (CUT + ACC) + 2.0 ** -22 * want_v.abs()
    swapped = idx != want_i
    assert bool(((got_v - want_v).abs() <= tol).all()), "a label out of place by more than the scan's bound"
    assert float(swapped.double().mean()) < 1e-3, "too many near-ties"
    # no label twice in a row
    s, _ = torch.sort(idx, dim=-1)
    assert bool((s[:, 1:] != s[:, :-1]).all())
    # probabilities: 1e-6, plus what the logits' own bound moves a softmax value by (|dp_j| <= 2 p_j (1 - p_j) max_i |dl_i|) --
    # fp32 logits of magnitude up to 100 are themselves only good to 2^-24 of that (6e-6)
    p64 = torch.softmax(lg, dim=-1).gather(1, idx)
    dl = (mag * (CUT + ACC) + 2.0 ** -22 * lg.abs()).max(dim=-1, keepdim=True).values
    assert bool(((prob.double() - p64).abs() <= 1e-6 + 2.0 * p64 * (1.0 - p64) * dl).all())
    # planted ties: wherever both twins are among the k, the smaller comes first
    for a, b in ((2, 5), (3, 70)):
        if b < text.shape[0]:
            pa = torch.where(idx == a, torch.arange(k, device=idx.device), k).min(dim=-1).values
            pb = torch.where(idx == b, torch.arange(k, device=idx.device), k).min(dim=-1).values
            both = (pa < k) & (pb < k)
            assert bool((pa[both] < pb[both]).all())


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("d", [64, 512, 100])
def test_topk_against_fp64(d, dtype):
    feats = _feats(50_000, d, dtype, seed=d)
    for nl in (1, 5, 20, 64, 65, 200, 512):
        text = _text(nl, d, seed=nl)
        for k in (1, 5, 8):
            if k > nl:
                continue
            idx, prob = E.topk_labels(feats, text, k=k)
            _check_topk(feats.float(), text, k, idx, prob)


def test_topk_planted_ties_put_the_smaller_label_first():
    d = 64
    g = torch.Generator().manual_seed(1)
    t = torch.randn(3, d, generator=g)
    t = t / t.norm(dim=-1, keepdim=True)
    text = torch.cat([t[0:1], t[1:2], t[1:2], t[2:3], t[1:2]] + [t[0:1]] * 70).cuda()  # label 1 = 2 = 4; 0 = 5.. 74
    feats = (t[1] * 3.0 + 0.01 * torch.randn(1000, d, generator=g)).cuda()  # every row closest to t[1]
    idx, _ = E.topk_labels(feats, text, k=3)
    assert bool((idx == torch.tensor([1, 2, 4], device="cuda")).all())
    feats = (t[0] * 3.0 + 0.01 * torch.randn(1000, d, generator=g)).cuda()
    idx, _ = E.topk_labels(feats, text, k=8)
    assert bool((idx == torch.tensor([0, 5, 6, 7, 8, 9, 10, 11], device="cuda")).all())


def test_topk_rejects_bad_k():
    feats = _feats(100, 64, "f32", 0)
    text = _text(5, 64, 0)
    for k in (0, 9, 6):
        with pytest.raises(ValueError):
            E.topk_labels(feats, text, k=k)
    from spatially_aware_ai_amd._lib import current_stream_ptr, lib

    out = torch.empty(100 * 9, dtype=torch.int32, device="cuda")
    for k in (0, 9, 6):
        rc = lib().saf_query_topk(feats.data_ptr(), _abi.SAF_F32, 100, 64, 64, text.data_ptr(), 5, 64, 100.0, _abi.SAF_NORM_L2_CLAMP,
                                  k, out.data_ptr(), None, None, 0, current_stream_ptr())
        assert rc == _abi.SAF_E_INVALID, k


def test_topk_top1_agrees_with_the_wide_row_argmax():
    from spatially_aware_ai_amd.clipfusion import query_scan_wide

    d, nl = 512, 200
    feats = _feats(50_000, d, "f16", 3)
    text = _text(nl, d, 4)
    text[5] = -text[5]  # (no planted tie here: the wide scan rounds the text to fp16)
    idx, _ = E.topk_labels(feats, text, k=1)
    aidx, _ = query_scan_wide(feats, text, "row_argmax", scale=100.0, normalize=True)
    f = feats.double()
    lg = f @ text.double().T
    lgh = f @ text.half().double().T  # the wide scan's scores: fp16 text
    top2 = torch.topk(lgh, 2, dim=-1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-3 * (f.abs() @ text.double().abs().T).max(dim=-1).values
    clear &= f.norm(dim=-1) > 0
    top2e = torch.topk(lg, 2, dim=-1).values
    clear &= (top2e[:, 0] - top2e[:, 1]) > 1e-3 * (f.abs() @ text.double().abs().T).max(dim=-1).values
    assert float(clear.double().mean()) > 0.9
    assert bool((idx[:, 0][clear] == aidx.long()[clear]).all())


def test_topk_exact_fp32_route_gives_the_same_indices(monkeypatch):
    feats = _feats(50_000, 512, "f32", 5)
    text = _text(200, 512, 6)
    a, pa = E.topk_labels(feats, text, k=5)
    monkeypatch.setenv("SAF_Q_SPLIT", "0")
    b, pb = E.topk_labels(feats, text, k=5)
    # the two routes differ by at most the split scan's bound: equal indices outside near-ties
    assert float((a != b).any(dim=-1).double().mean()) < 1e-3
    _check_topk(feats, text, 5, b, pb)


# ---------------------------------------------------------------------------------------------------- nearest neighbour
def _brute_nn(ref, query, chunk=64):
    r = ref.double()
    rx, ry, rz = r[:, 0][None], r[:, 1][None], r[:, 2][None]
    ar = torch.arange(r.shape[0], device=r.device)
    out_d, out_i = [], []
    for q in query.double().split(chunk):
        dx, dy, dz = q[:, 0:1] - rx, q[:, 1:2] - ry, q[:, 2:3] - rz
        d2 = dx * dx + dy * dy + dz * dz
        m = d2.min(dim=1).values
        out_d.append(m)
        out_i.append(torch.where(d2 == m[:, None], ar, r.shape[0]).min(dim=1).values)
    return torch.cat(out_i), torch.cat(out_d)


def _check_nn(ref, query, sample=None):
    idx, d2 = E.nearest_vertices(ref, query)
    assert idx.shape == (query.shape[0],) and d2.dtype == torch.float64
    if sample is not None:
        sel = torch.randperm(query.shape[0], generator=torch.Generator().manual_seed(0))[:sample].cuda()
        query, idx, d2 = query[sel], idx[sel], d2[sel]
    wi, wd = _brute_nn(ref, query)
    assert torch.equal(d2, wd), "distances differ from the fp64 brute force"
    assert torch.equal(idx, wi), "index is not the smallest at the nearest distance"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_nearest_uniform_with_duplicates():
    g = _gen(1)
    ref = torch.rand(100_000, 3, generator=g)
    ref[50_000:50_100] = ref[0:100]  # duplicated points: the smaller index
    query = torch.cat([torch.rand(20_000, 3, generator=g), ref[50_000:50_100], ref[:7]])
    _check_nn(ref.cuda(), query.cuda())


def test_nearest_clustered_blobs():
    g = _gen(2)
    centres = torch.randn(12, 3, generator=g) * 3
    ref = centres[torch.randint(0, 12, (80_000,), generator=g)] + 0.05 * torch.randn(80_000, 3, generator=g)
    query = centres[torch.randint(0, 12, (20_000,), generator=g)] + 0.3 * torch.randn(20_000, 3, generator=g)
    _check_nn(ref.cuda(), query.cuda())


def test_nearest_all_reference_points_identical():
    g = _gen(3)
    ref = torch.full((3000, 3), 0.25)
    query = torch.randn(2000, 3, generator=g)
    idx, d2 = E.nearest_vertices(ref.cuda(), query.cuda())
    assert bool((idx == 0).all())
    _check_nn(ref.cuda(), query.cuda())


def test_nearest_plane_and_far_queries():
    g = _gen(4)
    ref = torch.rand(200_000, 3, generator=g) * torch.tensor([4.0, 3.0, 0.0]) + torch.tensor([0.0, 0.0, 0.5])
    near = torch.rand(20_000, 3, generator=g) * torch.tensor([4.0, 3.0, 0.2]) + torch.tensor([0.0, 0.0, 0.4])
    far = torch.randn(2000, 3, generator=g) * 100.0
    _check_nn(ref.cuda(), torch.cat([near, far]).cuda())


def test_nearest_sizes_at_the_edges():
    g = _gen(5)
    q = torch.randn(500, 3, generator=g).cuda()
    _check_nn(torch.tensor([[0.5, -1.0, 2.0]]).cuda(), q)
    idx, d2 = E.nearest_vertices(torch.rand(10, 3).cuda(), torch.empty(0, 3).cuda())
    assert idx.numel() == 0 and d2.numel() == 0
    with pytest.raises(ValueError):
        E.nearest_vertices(torch.empty(0, 3).cuda(), q)
    with pytest.raises(ValueError):
        E.nearest_vertices(torch.tensor([[0.0, float("nan"), 0.0]]).cuda(), q)


def test_nearest_two_million_mesh_vertices():
    g = _gen(6)
    n, m = 2_000_000, 500_000
    # mesh-like: points on a sphere and the faces of a box, as the fused scans' vertices lie on surfaces
    s = torch.randn(n // 2, 3, generator=g)
    s = 0.9 * s / s.norm(dim=-1, keepdim=True)
    b = torch.rand(n - n // 2, 3, generator=g) * 2.4 - 1.2
    face = torch.randint(0, 6, (n - n // 2,), generator=g)
    b[torch.arange(b.shape[0]), face // 2] = torch.where(face % 2 == 0, -1.2, 1.2)
    ref = torch.cat([s, b]).cuda()
    query = (ref[torch.randint(0, n, (m,), generator=g).cuda()] + 0.01 * torch.randn(m, 3, generator=g).cuda())
    _check_nn(ref, query, sample=20_000)


# ---------------------------------------------------------------------------------------------------- counts
def _np_counts(gt, pred, c, topk):
    ok = (gt >= 0) & (gt < c)
    g, p = gt[ok], pred[ok]
    p0 = p[:, 0]
    in_range = (p0 >= 0) & (p0 < c)
    cmat = np.bincount(g[in_range] * c + p0[in_range], minlength=c * c).reshape(c, c)
    total = np.bincount(g, minlength=c)
    top1 = np.bincount(g[p0 == g], minlength=c)
    topk_ = np.bincount(g[(p[:, :topk] == g[:, None]).any(-1)], minlength=c)
    return cmat, top1, topk_, total


@pytest.mark.parametrize("c", [20, 200])
def test_counts_against_bincount(c):
    rng = np.random.default_rng(c)
    n = 300_000
    gt = rng.integers(-1, c + 3, n).astype(np.int32)
    pred = rng.integers(-1, c + 2, (n, 6)).astype(np.int32)
    pred[: n // 2, 0] = np.clip(gt[: n // 2], 0, c - 1)  # a classifier that is often right: hot diagonal bins
    got = E.segmentation_counts(torch.from_numpy(gt), torch.from_numpy(pred), c, topk=5)
    want = _np_counts(gt.astype(np.int64), pred.astype(np.int64), c, 5)
    for name, w in zip(("cmat", "ncorrect_top1", "ncorrect_topk", "ntotal"), want):
        assert np.array_equal(got[name].cpu().numpy(), w), name
    # accumulate over two halves == one call on the whole
    acc = E.segmentation_counts(torch.from_numpy(gt[: n // 3]), torch.from_numpy(pred[: n // 3]), c, topk=5)
    E.segmentation_counts(torch.from_numpy(gt[n // 3:]), torch.from_numpy(pred[n // 3:]), c, topk=5, into=acc)
    for name in got:
        assert torch.equal(acc[name], got[name]), name


# ---------------------------------------------------------------------------------------------------- end to end
class _StubClip:
    def __init__(self, text, prompts=None):
        self.text, self.prompts = text, prompts

    def text_inference(self, prompts):
        if self.prompts is not None:
            assert list(prompts) == list(self.prompts)
        return self.text


def _write_golden_scene(g, root):
    from spatially_aware_ai_amd import io

    scan = str(g["scan"])
    pred_dir, gt_dir = os.path.join(root, "pred", scan), os.path.join(root, "gt", scan)
    os.makedirs(pred_dir)
    os.makedirs(gt_dir)
    np.save(os.path.join(pred_dir, "vertex_clip_feats.npy"), g["feats"])
    io.save_ply(os.path.join(pred_dir, "mesh_rgb.ply"), g["pred_vertices"], np.zeros((0, 3), np.int32))
    faces = np.arange(3 * (len(g["gt_vertices"]) // 3), dtype=np.int32).reshape(-1, 3)
    io.save_ply(os.path.join(gt_dir, f"{scan}_vh_clean_2.ply"), g["gt_vertices"], faces)
    with open(os.path.join(gt_dir, f"{scan}.aggregation.json"), "w") as f:
        f.write(str(g["aggregation"]))
    with open(os.path.join(gt_dir, f"{scan}_vh_clean_2.0.010000.segs.json"), "w") as f:
        f.write(str(g["segs"]))
    return pred_dir, gt_dir


def test_eval_scene_equals_the_reference_golden(tmp_path):
    g = np.load(GOLDEN)
    labels, prompts = [str(s) for s in g["labels"]], [str(s) for s in g["prompts"]]
    pred_dir, gt_dir = _write_golden_scene(g, str(tmp_path))
    clip = _StubClip(torch.from_numpy(g["text"]), prompts)
    top, _ = E.segment(clip, os.path.join(pred_dir, "vertex_clip_feats.npy"), prompts)
    assert np.array_equal(top.cpu().numpy(), g["pred_top5"])
    idx, _ = E.nearest_vertices(g["pred_vertices"], g["gt_vertices"])
    assert np.array_equal(idx.cpu().numpy(), g["inds"])
    cmat, n1, n5, nt = E.eval_scene(pred_dir, gt_dir, labels, prompts, clip)
    assert cmat.dtype == np.int64 and np.array_equal(cmat, g["cmat"])
    assert np.array_equal(n1, g["ncorrect_top1"]) and np.array_equal(n5, g["ncorrect_top5"]) and np.array_equal(nt, g["ntotal"])
    assert np.array_equal(np.load(os.path.join(pred_dir, "gt_vertex_labels.npy")), g["gt_labels"])
    tr = np.load(os.path.join(pred_dir, "transferred_vertex_labels.npy"))
    assert tr.shape == (len(g["gt_vertices"]), 5) and np.array_equal(tr, g["pred_top5"][g["inds"]])
    s = E.summarize(cmat, n1, n5, nt)
    np.testing.assert_allclose(s["iou"], g["iou"], rtol=0, atol=1e-12, equal_nan=True)
    for a, b in (("miou", "miou"), ("macc_top1", "macc_top1"), ("macc_topk", "macc_top5")):
        assert abs(s[a] - float(g[b])) <= 1e-12, a
    # the __main__ loop over the one scene
    res = E.evaluate(os.path.join(str(tmp_path), "pred"), os.path.join(str(tmp_path), "gt"), labels, prompts, lambda d: clip)
    assert abs(res["miou"] - float(g["miou"])) <= 1e-12
    assert np.array_equal(np.load(os.path.join(str(tmp_path), "pred", "global_cmat.npy")), g["cmat"])
    with open(os.path.join(str(tmp_path), "pred", "scene_cmats.json")) as f:
        assert json.load(f) == {str(g["scan"]): g["cmat"].tolist()}


def test_segment_raises_on_non_finite_features():
    g = np.load(GOLDEN)
    clip = _StubClip(torch.from_numpy(g["text"]))
    f = g["feats"].copy()
    f[7, 3] = np.nan
    with pytest.raises(ValueError, match="found nans"):
        E.segment(clip, f, list(g["prompts"]))
    f[7, 3] = np.inf
    with pytest.raises(ValueError, match="found nans"):
        E.segment(clip, f, list(g["prompts"]))


def _fused_scan_mesh():
    from spatially_aware_ai_amd import synthetic as syn
    from spatially_aware_ai_amd.scene import reconstruct_scene

    w, h, d = 64, 48, 64
    scan = syn.SyntheticScan(21, 60, w, h, d)
    names, colors = syn.scene_class_names(), syn.scene_class_colors()
    clip, seg = syn.ReplayClip(scan, class_names=names), syn.ReplaySeg(scan)
    config = {"voxel_size": 0.04, "trunc_vox": 3, "clip_patch_size": scan.patch, "clip_patch_stride": scan.stride}
    res = reconstruct_scene(scan, config, clip, seg, names, colors, out_dir=None)
    verts, faces, _, feats = res.fusion.extract_mesh()[:4]
    return scan, res.fusion, torch.as_tensor(verts).float(), feats


def test_a_fused_scan_scores_well():
    from spatially_aware_ai_amd import synthetic as syn

    scan, fz, verts, feats = _fused_scan_mesh()
    nvox = [int(v) for v in fz.nvox]
    assert 64 <= max(nvox) <= 96, nvox
    classes = list(dict.fromkeys(syn.SCENE_SURFACE_CLASSES))  # distinct, renumbered 0..n-1
    n_cls = len(classes)
    # GT: points on the analytic sphere (surface 0) and the box's faces (1..6: -x +x -y +y -z +z), with their class
    g = torch.Generator().manual_seed(9)
    s = torch.randn(4000, 3, generator=g)
    s = 0.9 * s / s.norm(dim=-1, keepdim=True)
    b = torch.rand(12000, 3, generator=g) * 2.4 - 1.2
    face = torch.randint(0, 6, (12000,), generator=g)
    b[torch.arange(12000), face // 2] = torch.where(face % 2 == 0, -1.2, 1.2)
    gt_v = torch.cat([s, b])
    surface = torch.cat([torch.zeros(4000, dtype=torch.long), 1 + face])
    gt = torch.tensor([classes.index(syn.SCENE_SURFACE_CLASSES[i]) for i in surface.tolist()], dtype=torch.int32)
    # keep the GT points the scan saw (within 5 cm of its mesh)
    _, d2 = E.nearest_vertices(verts, gt_v)
    seen = (d2 < 0.05 ** 2).cpu()
    gt_v, gt = gt_v[seen], gt[seen]
    assert len(gt) > 2000

    def run(text):
        labels, _ = E.segment(_StubClip(text), feats, [f"c{i}" for i in range(n_cls)], k=5)
        transferred = E.transfer_labels(verts, gt_v, labels)
        c = E.segmentation_counts(gt, transferred, n_cls, topk=5)
        # numpy restatement: brute-force nearest vertex, then the counts
        wi, _ = _brute_nn(verts.cuda(), gt_v.cuda(), chunk=256)
        want = _np_counts(gt.numpy().astype(np.int64), labels[wi].cpu().numpy(), n_cls, 5)
        for name, w in zip(("cmat", "ncorrect_top1", "ncorrect_topk", "ntotal"), want):
            assert np.array_equal(c[name].cpu().numpy(), w), name
        return E.summarize(c["cmat"], c["ncorrect_top1"], c["ncorrect_topk"], c["ntotal"])

    good = run(scan.emb[classes])
    rand = torch.randn(n_cls, scan.emb.shape[1], generator=torch.Generator().manual_seed(1))
    bad = run(rand / rand.norm(dim=-1, keepdim=True))
    print("fused scan: mIoU", good["miou"], "mAcc", good["macc_top1"], "| random text: mIoU", bad["miou"])
    # measured on the MI355X: mIoU 0.68, mAcc 0.77 with the classes' own embeddings; random text vectors 0.17.  The feature map's
    # cells are 16-pixel patches at a stride of 8 on a 64 x 48 image, so class boundaries are blurred over several voxels.
    assert good["miou"] > 0.6 and good["macc_top1"] > 0.7
    assert bad["miou"] < 0.3
