"""CPU: the ray-cast contract on its NumPy restatement (tests/raycast_reference.py) and the host side of the two entry points.

  * fragile pixels -- where the float64 and the float32 run of the restatement disagree on hit / miss, crossing interval or
    voxel -- are at most 1 % of every test view (the GPU tests exclude them; a view that had more would be replaced);
  * the float64 restatement against the analytic depth of the scene: the 99th percentile of |depth - analytic| on
    silhouette-free pixels, in voxels, is printed (DESIGN.md 4.13 quotes it; tests/test_raycast_gpu.py measures the same figure
    again as the baseline of its analytic test) and lies below the truncation distance;
  * front faces only: no view reports a depth nearer than the analytic depth minus the truncation distance on silhouette-free
    pixels, and the view through a wall (no silhouette in it) on any pixel, although every ray crosses the near wall from behind;
  * saf_raycast / saf_gather_rows refuse bad arguments on the host (no GPU needed: nothing is launched);
  * the edge scene (raycast_reference.edge_scene / edge_views, a hand-written 20 x 24 x 28 volume): the restatement alone meets
    what tests/test_raycast_edges.py relies on -- at most 2 % fragile pixels per case, hits in the last cell of z, a hole that
    breaks rays to the floor, hits on voxels without colour, all misses where nothing can be seen.
"""
import ctypes

import numpy as np
import pytest

import raycast_reference as rr
from host_stubs import fake_volume as _fake_volume
from spatially_aware_ai_amd import _abi, _lib
from spatially_aware_ai_amd import synthetic as syn

FRAGILE_CAP = 0.01
EDGE_FRAGILE_CAP = 0.02


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


# ---- the edge scene
def _edge_cases():
    return [c[0] for c in rr.edge_views()]


def test_edge_scene_is_what_the_device_tests_assume():
    sc = rr.edge_scene()
    nx, ny, nz = sc["nvox"]
    assert (nx, ny, nz) == (20, 24, 28) and len({nx, ny, nz}) == 3, "a grid with two equal sides hides a swap of them"
    n = nx * ny * nz
    assert sc["tsdf"].shape == (n,) and sc["tsdf"].dtype == np.float32 and sc["tsdf_weight"].dtype == np.int32
    assert sc["weight"].dtype == np.int32 and sc["rgb"].shape == (n, 3) and sc["rgb"].dtype == np.float32
    assert sc["rgb"].min() >= 0 and sc["rgb"].max() < 1
    for a, tab in enumerate(sc["axes"]):  # exact in fp32: voxel size and origin are multiples of 1 / 16
        assert tab.dtype == np.float32 and np.array_equal(tab.astype(np.float64), rr.E_ORG[a] + rr.E_VS * np.arange(sc["nvox"][a]))
    tw, wt = sc["tsdf_weight"].reshape(sc["nvox"]), sc["weight"].reshape(sc["nvox"])
    assert tw.sum() == 18 * 22 * 26 - 3 * 4 * 4 and (tw[rr.E_HOLE] == 0).all() and tw[1, 1, 27] == 1 and tw[0].sum() == 0
    assert (wt == 0).sum() == 300 and (tw[rr.E_UNCOLOURED] == 1).all(), "the uncoloured patch is observed"
    # 16 x 16-pixel blocks per inside size: 8 + a remainder, fewer than 8, single blocks
    blocks = [-(-w // 16) * -(-h // 16) for w, h in rr.E_INSIDE_SIZES]
    assert blocks == [12, 26, 6, 6, 1, 1, 1, 1]


def test_edge_fragile_pixels_are_rare():
    _, runs = rr.edge_reference()
    for name in _edge_cases():
        c = rr.edge_counts(name)
        fr = c["fragile"]
        print(f"{name}: {c['pixels']} pixels, {c['hits']} hits, {int(fr.sum())} fragile ({fr.mean():.4%}), {int(c['last_cell'].sum())} in the last "
              f"cell of z, {int(c['hole_broken'].sum())} of {int(c['hole'].sum())} over the hole broken, {int(c['uncoloured'].sum())} on weight == 0")
        assert fr.size == c["pixels"] and fr.mean() <= EDGE_FRAGILE_CAP, f"{name}: {fr.mean():.3%} fragile pixels; move the hole or the camera"


def test_edge_cases_are_not_vacuous():
    _, runs = rr.edge_reference()
    c = rr.edge_counts("inside_61x45")
    assert c["hits"] > 0.9 * c["pixels"]
    assert c["last_cell"].sum() >= 50, "too few hits in the last cell of z"
    assert c["hole_broken"].sum() >= 20 and c["hole_broken"].sum() == c["hole"].sum(), "the hole does not break the rays to the floor under it"
    assert c["uncoloured"].sum() >= 50, "too few hits on voxels with weight == 0"
    # the same rays reach the floor without the hole: it is the hole that breaks them
    sc = rr.edge_scene(hole=False)
    _, pose, k, h, w, kw = rr.edge_views()[0]
    whole = rr.raycast(sc["tsdf"], sc["tsdf_weight"], sc["axes"], pose, k, h, w, **kw)
    assert (whole["hit"] & (whole["voxel"] % 28 >= 26))[c["hole"]].all()
    for name in ("inside_8x8", "inside_5x3", "inside_1x1", "axis_aligned", "axis_aligned_off", "outside"):
        assert runs[name][0]["hit"].any(), name
    assert rr.edge_counts("outside")["uncoloured"].sum() >= 50  # (the wall x = 17.5 square on)


def test_edge_axis_aligned_view():
    """Identity rotation: column 10 has dx == 0 and row 8 dy == 0 exactly, in both precisions; the centre pixel looks straight
    down z at the floor, 26.4 - 5 = 21.4 voxels away."""
    _, runs = rr.edge_reference()
    _, pose, k, h, w, _ = next(c for c in rr.edge_views() if c[0] == "axis_aligned")
    assert (h, w) == (17, 21) and np.array_equal(pose[:3, :3], np.eye(3, dtype=np.float32)) and k[0, 2] == 10 and k[1, 2] == 8
    r64, r32 = runs["axis_aligned"]
    fr = rr.fragile(r64, r32)
    assert not fr[:, 10].any() and not fr[8, :].any()
    assert r64["hit"][8, 10] and abs(r64["depth"][8, 10] / rr.E_VS - 21.4) < 1e-7, r64["depth"][8, 10] / rr.E_VS
    assert r64["hit"][:, 10].sum() >= 10 and r64["hit"][8, :].sum() >= 10, "the axis-parallel rays see nothing"


def test_edge_nothing_to_see_is_all_misses():
    _, runs = rr.edge_reference()
    for name in ("nothing", "degenerate_fx0", "degenerate_nan", "degenerate_inf"):
        for r in runs[name]:
            assert not r["hit"].any() and (r["depth"] == 0).all() and (r["voxel"] == -1).all(), name


def test_edge_near_and_far_planes():
    _, runs = rr.edge_reference()
    for r in runs["inside_61x45_near0.3_far0.9"]:
        hit = r["hit"]
        assert hit.sum() > 100 and (~hit).sum() > 100
        assert (r["depth"][hit] >= np.float32(0.3)).all() and (r["depth"][hit] <= np.float32(0.9)).all()
    # the near plane alone changes where the samples fall, not what is seen
    a, b = runs["inside_61x45"][0], runs["inside_61x45_near0.3"][0]
    assert (a["hit"] == b["hit"]).mean() > 0.99 and (b["depth"][b["hit"]] >= np.float32(0.3)).all()
