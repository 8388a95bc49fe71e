#!/usr/bin/env python3
"""Benchmark of saf_label_components (the connected-component core of
flood_fill_3d, handy_utils.py:295-480) on a synthetic label grid.

    python bench_components.py [--grid 256] [--classes 40] [--iters 10]

Prints one JSON line: voxels/s of the HIP path (HIP-event timed, inputs resident), its algorithmic bytes
(labels read once + object ids written once, 8 B per voxel) against the HBM peak, and the oracle's C
restatement of the reference's raster-scan flood fill timed on a smaller grid as the CPU baseline (the
reference itself is a pure-Python triple loop)."""
import argparse
import json
import time

import torch

HBM_PEAK_GBS = 8000.0


def synthetic_labels(n, classes, seed=0):
    """Blobby label field: class = quantised sum of a few low-frequency waves; ~35 % empty, ~5 % null."""
    g = torch.Generator().manual_seed(seed)
    ax = torch.linspace(0, 1, n)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    f = torch.zeros(n, n, n)
    for _ in range(6):
        k = torch.rand(3, generator=g) * 14 + 2
        p = torch.rand(3, generator=g) * 6.28
        f += torch.sin(k[0] * x + p[0]) * torch.sin(k[1] * y + p[1]) * torch.sin(k[2] * z + p[2])
    q = ((f - f.min()) / (f.max() - f.min()) * classes).long().clamp_(0, classes - 1).to(torch.int32)
    r = torch.rand(n, n, n, generator=g)
    q[f.abs() < 0.25] = -1
    q[r < 0.05] = 133
    return q


def bench_mesh(a):
    """extract_mesh() (clipfusion.py:723-763) on a fused volume: 64 frames of the coherent synthetic
    scene (sphere in a box) into a grid^3 x 512 volume, then marching cubes on the TSDF and the trilinear sampling of
    colours and D-dim features at the vertices -- all on the device, nothing but the mesh leaves it."""
    import bench
    from spatially_aware_ai_amd import ClipFusion
    from spatially_aware_ai_amd import synthetic as syn

    class R:
        feature_dim = 512

    dev = torch.device("cuda", 0)
    g = syn.make_grid(a.grid)
    npy, npx = syn.feature_map_shape(640, 480)
    depth, rgb, poses, ks, feat = bench.gen_frames_gpu(64, 640, 480, 512, npy, npx, "B", 1000, dev)
    fz = ClipFusion(g.origin, g.voxel_size, g.nvox, g.trunc, False, R(), None, 160, 80, keep_xyz_world=False).to(dev)
    fz.integrate_features(depth, rgb, poses, ks, feat)
    fz.flush()
    out = fz.extract_mesh()  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        del out  # (1.5 GB of vertex features: the allocator reuses the block instead of asking the driver for a second one)
        out = fz.extract_mesh()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.iters * 1e3
    verts, faces = out[0], out[1]
    n = int(fz.tsdf.numel())
    nv, nf = int(len(verts)), int(len(faces))
    # algorithmic bytes: tsdf + weight read once (8 B per voxel), per vertex 8 corner rows of D features + rgb, outputs
    alg = n * 8 + nv * (8 * (512 * 4 + 12) + 512 * 4 + 12 + 12) + nf * 24
    print(json.dumps({
        "metric": f"extract_mesh of a {a.grid}^3 x 512 volume (marching cubes + vertex colours and features)", "value": round(ms, 3),
        "unit": "ms", "higher_is_better": False, "vertices": nv, "faces": nf, "dtype": "f32", "data": "synthetic (64 frames, scene B)",
        "roofline": {"bound": "hbm", "achieved": round(alg / ms / 1e6, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": round(alg / ms / 1e6 / HBM_PEAK_GBS, 4), "traffic": None,
                     "note": "includes the device -> host copy of the mesh (vertices, faces as numpy; colours and features stay "
                             "tensors) and the host-side glue of extract_mesh()"}}))


def bench_pose(a):
    """refine_pose() (saf_pose_refine) of a 640 x 480 depth frame against a grid^3 volume fused from 16 frames of the
    coherent synthetic scene, default levels ((4, 6), (2, 4), (1, 4)): the frame is one of the fused ones, its pose moved by a
    voxel and by a rotation that moves the scene by a voxel.  Device events around --iters calls, three windows (the spread);
    "all_steps" is the same call with zero tolerances, so that none of the 14 steps is skipped."""
    import numpy as np

    import bench
    from spatially_aware_ai_amd import ClipFusion
    from spatially_aware_ai_amd import synthetic as syn

    class R:
        feature_dim = 64

    dev = torch.device("cuda", 0)
    g = syn.make_grid(a.grid)
    npy, npx = syn.feature_map_shape(640, 480)
    depth, rgb, poses, ks, feat = bench.gen_frames_gpu(16, 640, 480, 64, npy, npx, "B", 1000, dev)
    fz = ClipFusion(g.origin, g.voxel_size, g.nvox, g.trunc, False, R(), None, 160, 80, keep_xyz_world=False).to(dev)
    fz.integrate_features(depth, rgb, poses, ks, feat)
    fz.flush()
    vs = float(g.voxel_size)
    pose = poses[0].double().cpu()
    w = torch.tensor([0.6, -0.5, 0.62], dtype=torch.float64) * (vs / float(depth[0].max()))
    wx = torch.tensor([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=torch.float64)
    pose[:3, :3] = torch.linalg.matrix_exp(wx) @ pose[:3, :3]
    pose[:3, 3] += torch.tensor([0.6, 0.64, -0.48], dtype=torch.float64) * vs
    pose = pose.float().to(dev)
    out = {}
    for name, kw in (("default", {}), ("all_steps", {"tol_t": 0.0, "tol_r": 0.0})):
        for _ in range(5):  # warm-up
            res = fz.refine_pose(depth[0], pose, ks[0], **kw)
        torch.cuda.synchronize()
        ms = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                res = fz.refine_pose(depth[0], pose, ks[0], **kw)
            e1.record()
            torch.cuda.synchronize()
            ms.append(round(e0.elapsed_time(e1) / a.iters, 4))
        log = res.log.cpu().numpy()
        out[name] = {"ms": ms, "status": int(res.status), "steps": int((log[:, 0] > 0).sum()), "n_valid": res.n_valid,
                     "moved_voxels": round(float((res.pose[:3, 3] - pose[:3, 3]).norm()) / vs, 4)}
    print(json.dumps({
        "metric": f"refine_pose of a 640 x 480 frame against a {a.grid}^3 volume (default levels)", "value": min(out["default"]["ms"]),
        "unit": "ms", "higher_is_better": False, "iters": a.iters, "dtype": "f32 chain, f64 sums", "data": "synthetic (16 frames, scene B)",
        "runs": out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--classes", type=int, default=40)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--cpu-grid", type=int, default=96)
    ap.add_argument("--mesh", action="store_true", help="time extract_mesh (marching cubes + vertex sampling) instead")
    ap.add_argument("--pose", action="store_true", help="time refine_pose (the device Gauss-Newton against the TSDF) instead")
    a = ap.parse_args()
    if a.mesh:
        return bench_mesh(a)
    if a.pose:
        return bench_pose(a)
    from spatially_aware_ai_amd import label_components

    lab = synthetic_labels(a.grid, a.classes).cuda()
    ids, first, cls, cnt = label_components(lab)  # warm-up (also sizes the workspace allocator)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        ids, first, cls, cnt = label_components(lab)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.iters
    n = lab.numel()
    cpu = None
    try:
        from oracle import oracle as O

        small = synthetic_labels(a.cpu_grid, a.classes).numpy()
        t0 = time.perf_counter()
        O.label_components(small)
        dt = time.perf_counter() - t0
        cpu = {"value": round(small.size / dt / 1e6, 2), "unit": "Mvoxels/s", "cores": 1, "kind": "port",
               "sample": f"{a.cpu_grid}^3 grid, oracle/saf_oracle.c raster-scan flood fill (1 thread)"}
    except Exception as e:  # the oracle is optional
        cpu = {"value": None, "sample": f"unavailable: {e}"}
    print(json.dumps({
        "metric": f"label components of a {a.grid}^3 grid", "value": round(n / ms / 1e3, 1), "unit": "Mvoxels/s",
        "ms": round(ms, 3), "objects": int(first.numel()), "largest": int(cnt.max()) if cnt.numel() else 0,
        "dtype": "int32", "data": "synthetic",
        "roofline": {"bound": "hbm", "achieved": round(n * 8 / ms / 1e6, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": round(n * 8 / ms / 1e6 / HBM_PEAK_GBS, 4), "traffic": None,
                     "note": "algorithmic = labels read once + ids written once; the union-find passes re-read parent[] "
                             "(4 more N x 4 B arrays live in the workspace)"},
        "cpu_baseline": cpu}))


if __name__ == "__main__":
    main()
