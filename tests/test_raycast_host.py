"""CPU: the ray-cast contract on its NumPy restatement (tests/raycast_reference.py) and the host side of the two entry points.

  * fragile pixels -- where the float64 and the float32 run of the restatement disagree on hit / miss, crossing interval or
    voxel -- are at most 1 % of every test view (the GPU tests exclude them; a view that had more would be replaced);
  * the float64 restatement against the analytic depth of the scene: the 99th percentile of |depth - analytic| on
    silhouette-free pixels, in voxels, is printed (DESIGN.md 4.13 quotes it; tests/test_raycast_gpu.py measures the same figure
    again as the baseline of its analytic test) and lies below the truncation distance;
  * front faces only: no view reports a depth nearer than the analytic depth minus the truncation distance on silhouette-free
    pixels, and the view through a wall (no silhouette in it) on any pixel, although every ray crosses the near wall from behind;
  * saf_raycast / saf_gather_rows refuse bad arguments on the host (no GPU needed: nothing is launched).
"""
import ctypes

import numpy as np
import pytest

import raycast_reference as rr
from spatially_aware_ai_amd import _abi, _lib
from spatially_aware_ai_amd import synthetic as syn

FRAGILE_CAP = 0.01


@pytest.fixture(scope="module")
def fused(oracle):
    """The scene fused by the CPU oracle, and per view the two runs of the restatement."""
    sc = rr.scan()
    grid = syn.make_grid(rr.NVOX, trunc_vox=rr.TRUNC_VOX)
    vol = oracle.OracleVolume(grid.origin, grid.voxel_size, grid.nvox, grid.trunc, rr.DIM, 143)
    oracle.set_threads(8)
    try:
        for f in sc.frames:
            vol.integrate(f["depth"], f["rgb"], f["pose"], f["K"], f["feat"], [f["labels"].float()], rgb_bilinear=True)
    finally:
        oracle.set_threads(1)
    axes = [a.numpy() for a in vol.axes]
    zf = rr.grid_diagonal(grid.voxel_size, [int(v) for v in grid.nvox])
    runs = {}
    for name, pose, k in rr.views():
        w, h = rr.WH
        r64, r32 = (rr.raycast(vol.tsdf.numpy(), vol.tsdf_weight.numpy(), axes, pose.numpy(), k.numpy(), h, w, z_far=zf, dtype=dt)
                    for dt in (np.float64, np.float32))
        runs[name] = (pose, k, r64, r32)
    return grid, vol, runs


def test_views_see_the_scene(fused):
    _, _, runs = fused
    for name, (_, _, r64, _) in runs.items():
        share = r64["hit"].mean()
        print(f"{name}: {share:.3f} of the pixels hit")
        assert share > 0.3, f"view {name} hardly sees the volume"


def test_fragile_pixels_are_rare(fused):
    _, _, runs = fused
    for name, (_, _, r64, r32) in runs.items():
        fr = rr.fragile(r64, r32)
        print(f"{name}: {int(fr.sum())} fragile pixels of {fr.size} ({fr.mean():.4%})")
        assert fr.mean() <= FRAGILE_CAP, f"view {name}: {fr.mean():.3%} fragile pixels; choose another view"


def test_reference_against_the_analytic_depth(fused):
    grid, _, runs = fused
    for name, (pose, k, r64, _) in runs.items():
        depth, surface = rr.analytic(pose, k)
        m = r64["hit"] & (depth > 0) & rr.constant_surface(surface)
        assert m.sum() > 1000, name
        err = np.abs(r64["depth"][m] - depth[m]) / grid.voxel_size
        p99 = float(np.percentile(err, 99))
        print(f"{name}: float64 reference vs analytic depth on {int(m.sum())} silhouette-free pixels: p99 = {p99:.4f} voxels, "
              f"max = {err.max():.4f}")
        assert p99 < rr.TRUNC_VOX, f"view {name}: p99 depth error {p99:.3f} voxels is not inside the truncation band"


def test_front_faces_only(fused):
    """Every ray of these views crosses the near wall from behind (negative to positive): not a hit.  On silhouette-free pixels
    no depth is nearer than the analytic depth minus the truncation distance; the view through the wall has no silhouette (all
    of its rays land on the sphere), and there the bound holds on EVERY pixel."""
    grid, _, runs = fused
    for name, (pose, k, r64, r32) in runs.items():
        depth, surface = rr.analytic(pose, k)
        for r in (r64, r32):
            m = r["hit"] & (depth > 0) & rr.constant_surface(surface)
            early = r["depth"][m] < depth[m] - grid.trunc
            assert not early.any(), f"view {name}: {int(early.sum())} pixels report a surface in front of the scene (the near wall's back?)"
    pose, k, r64, r32 = runs["through_wall"]
    depth, surface = rr.analytic(pose, k)
    assert (surface == 0).all() and (depth > 0).all(), "the view through the wall is meant to see nothing but the sphere"
    for r in (r64, r32):
        assert r["hit"].mean() > 0.8
        early = r["hit"] & (r["depth"] < depth - grid.trunc)
        assert not early.any(), f"{int(early.sum())} pixels of the view through the wall report a surface in front of the scene"


def test_unsupported_intrinsics_are_all_misses(fused):
    """A K with skew, or a third row other than (0, 0, 1): the contract reports every pixel as a miss."""
    _, vol, runs = fused
    pose, k, _, _ = runs["rolled"]
    axes = [a.numpy() for a in vol.axes]
    w, h = rr.WH
    for (i, j), val in (((0, 1), 0.5), ((1, 0), -0.1), ((2, 0), 1e-3), ((2, 2), 2.0)):
        bad = k.clone()
        bad[i, j] = val
        r = rr.raycast(vol.tsdf.numpy(), vol.tsdf_weight.numpy(), axes, pose.numpy(), bad.numpy(), h, w, dtype=np.float32)
        assert not r["hit"].any() and (r["depth"] == 0).all() and (r["voxel"] == -1).all()


def _fake_volume(n=8):
    v = _abi.SafVolume()
    v.nx = v.ny = v.nz = n
    for f in ("axis_x", "axis_y", "axis_z", "tsdf", "tsdf_weight", "weight", "rgb", "clip_feat"):
        setattr(v, f, 4096)  # non-NULL, aligned: the descriptor is only inspected
    return v


def test_raycast_rejects_bad_arguments_on_the_host():
    l = _lib.lib()
    vol = _fake_volume()
    p = 4096  # a non-NULL stand-in for a device pointer; every call below must fail before it would be used
    good = dict(vol=ctypes.byref(vol), pose=p, K=p, h=4, w=4, step=0.5, zn=0.0, zf=3.0, depth=p, voxel=p)
    bad = [dict(vol=None), dict(pose=None), dict(K=None), dict(depth=None), dict(voxel=None), dict(h=0), dict(w=-3), dict(step=0.0),
           dict(step=-1.0), dict(step=float("nan")), dict(zf=0.0), dict(zn=1.0, zf=1.0), dict(vol=ctypes.byref(_abi.SafVolume())),
           dict(vol=ctypes.byref(_fake_volume(1)))]
    for change in bad:
        a = dict(good, **change)
        rc = l.saf_raycast(a["vol"], a["pose"], a["K"], a["h"], a["w"], a["step"], a["zn"], a["zf"], a["depth"], a["voxel"], None, None)
        assert rc == _abi.SAF_E_INVALID, change
        assert b"raycast" in l.saf_last_error()


def test_gather_rows_rejects_bad_arguments_on_the_host():
    l = _lib.lib()
    p = 4096
    good = dict(src=p, n=10, rb=64, idx=p, ni=5, dst=p)
    bad = [dict(src=None), dict(idx=None), dict(dst=None), dict(n=0), dict(ni=0), dict(ni=-1), dict(rb=0), dict(rb=24), dict(rb=4),
           dict(rb=-16), dict(src=4100), dict(dst=4104)]
    for change in bad:
        a = dict(good, **change)
        rc = l.saf_gather_rows(a["src"], a["n"], a["rb"], a["idx"], a["ni"], a["dst"], None)
        assert rc == _abi.SAF_E_INVALID, change
        assert b"gather rows" in l.saf_last_error()


def test_render_has_no_cpu_fallback():
    import torch

    from spatially_aware_ai_amd import clipfusion

    class FakeClip:
        feature_dim = 8

    f = clipfusion.ClipFusion(torch.zeros(3), 0.1, torch.tensor([4, 4, 4]), 0.3, False, FakeClip(), None, 10, 10)
    with pytest.raises(_lib.SafError, match="no CPU fallback"):
        f.render(torch.eye(4), torch.eye(3), 30, 40)
    with pytest.raises(_lib.SafError, match="no CPU fallback"):
        f.render_query(torch.zeros(2, 8), torch.eye(4), torch.eye(3), 30, 40)
