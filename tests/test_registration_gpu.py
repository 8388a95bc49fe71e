"""GPU: the rig front-end (saf_undistort_images, saf_depth_to_color, saf_color_to_depth; registration.py) against the NumPy
restatement of its contract (tests/registration_reference.py), the analytic scene, and into the fusion.

Bars (none of them taken from the device's output; tests/test_registration_host.py checks on the restatement alone that the rigs
meet the conditions these rely on):
  * indices, validity and hit / miss equal the float64 restatement on non-fragile pixels, with at most twice as many exceptions
    as there are fragile pixels; values on agreeing pixels within 4 x the largest float32-vs-float64 gap of the restatement
    itself on the same mask (the margin of tests/test_raycast_gpu.py for the same kind of comparison);
  * missing depth (0, NaN, +-inf, negative) gives 0 / invalid, never a value; the identity rig is the identity bit for bit;
  * two calls return the same bytes;
  * against the analytic scene the device's p99 relative depth error is at most the float64 restatement's plus the gap above;
  * on rig C's analytically occluded band the device marks at least the restatement's share invalid, and with the test off
    the same pixels are valid and carry the sphere's colour;
  * a volume fused from registered frames renders within the ideal-frame volume's error plus the registration error.
"""
import numpy as np
import pytest
import torch

import registration_reference as rr
from spatially_aware_ai_amd import registration as reg
from spatially_aware_ai_amd import synthetic as syn

pytestmark = pytest.mark.gpu


def _np(t):
    return t.cpu().numpy()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device(r, zbuf_on=True):
    """The three entry points on a rig: dict of numpy arrays, plus the occlusion tolerance used."""
    d, rgb, T = _cuda(r.depth), _cuda(r.rgb), _cuda(r.T_d2c)
    splat = reg.depth_to_color(d, r.depth_cam, T, r.color_cam)
    tol = rr.occlusion_tol(_np(splat))
    gd, grgb, gvalid = reg.color_to_depth(d, r.depth_cam, T, rgb, r.color_cam, zbuf=splat if zbuf_on else None, occlusion_tol=tol)
    hd, wd = r.depth_cam.height, r.depth_cam.width
    own_index = torch.arange(1, hd * wd + 1, dtype=torch.float32).reshape(1, hd, wd).cuda()  # (exact in f32: < 2^24)
    out = dict(splat=_np(splat), undistort_rgb=_np(reg.undistort(rgb, r.color_cam, reg.BILINEAR)),
               undistort_depth=_np(reg.undistort(d, r.depth_cam, reg.NEAREST)),
               nearest_index=_np(reg.undistort(own_index, r.depth_cam, reg.NEAREST))[0].astype(np.int64) - 1,
               gather_depth=_np(gd), gather_rgb=_np(grgb), gather_valid=_np(gvalid))
    torch.cuda.synchronize()
    return out, tol


@pytest.fixture(scope="module")
def on_device():
    """Per rig: (the device's outputs, the two restatement runs fed the DEVICE's splat as z-buffer, the tolerance)."""
    out = {}
    for name in ("A", "B"):
        r = rr.rig(name)
        dev, tol = _device(r)
        runs, tol_r = rr.runs(r, zbuf=dev["splat"])
        assert tol == tol_r
        out[name] = (dev, runs)
    return out


def _values_close(what, dev, r64, r32, mask):
    assert mask.sum() > 0.3 * mask.size, f"{what}: only {int(mask.sum())} pixels to compare"
    with np.errstate(invalid="ignore"):
        gap = float(np.abs(r32.astype(np.float64) - r64)[mask].max())
        err = float(np.abs(dev.astype(np.float64) - r64)[mask].max())
    print(f"{what}: values on {int(mask.sum())} agreeing pixels: device-vs-f64 max {err:.3e}, restatement f32-vs-f64 max {gap:.3e}; "
          f"device == f32 restatement bit for bit on {int((dev[mask] == r32[mask]).sum())} of {int(mask.sum())}")
    assert err <= 4 * gap, f"{what}: off by {err:.3e}, the restatement's own fp32 gap is {gap:.3e}"


def _count(what, differ, fr):
    print(f"{what}: {int(fr.sum())} fragile pixels, {int(differ.sum())} non-fragile pixels differ from float64")
    assert differ.sum() <= 2 * fr.sum(), f"{what}: {int(differ.sum())} non-fragile pixels differ, {int(fr.sum())} fragile ones"


@pytest.mark.parametrize("name", ["A", "B"])
def test_splat_against_the_reference(on_device, name):
    dev, runs = on_device[name]
    r64, r32 = runs["splat"]
    fr = rr.fragile("splat", r64, r32)
    got = dev["splat"]
    assert np.isfinite(got).all() and (got >= 0).all()
    hit, hit64 = got > 0, r64["depth"] > 0
    _count(f"rig {name} splat", (hit != hit64) & ~fr, fr)
    _values_close(f"rig {name} splat", got, r64["depth"], r32["depth"], hit & hit64 & (r32["depth"] > 0) & ~fr)


@pytest.mark.parametrize("name", ["A", "B"])
def test_undistort_against_the_reference(on_device, name):
    dev, runs = on_device[name]
    r = rr.rig(name)
    r64, r32 = runs["undistort_depth"]
    fr = r64["index"] != r32["index"]
    _count(f"rig {name} undistort nearest", (dev["nearest_index"] != r64["index"]) & ~fr, fr)
    same = dev["nearest_index"] == r64["index"]
    want = r64["out"][..., 0].astype(np.float32)  # a gather: the source's own bits (NaN and inf included)
    assert np.array_equal(dev["undistort_depth"][:, same], want[:, same], equal_nan=True)
    assert (dev["undistort_depth"][:, dev["nearest_index"] < 0] == 0).all()
    r64, r32 = runs["undistort_rgb"]
    assert dev["undistort_rgb"].shape == (r.rgb.shape[0], r.color_cam.height, r.color_cam.width, 3)
    _values_close(f"rig {name} undistort bilinear", dev["undistort_rgb"], r64["out"], r32["out"], np.ones(r64["out"].shape, dtype=bool))


@pytest.mark.parametrize("name", ["A", "B"])
def test_gather_against_the_reference(on_device, name):
    dev, runs = on_device[name]
    r64, r32 = runs["gather"]
    fr = rr.fragile("gather", r64, r32)
    d64 = r64["depth"].astype(np.float32)
    differ = ((dev["gather_valid"] != r64["valid"]) | (dev["gather_depth"] != d64)) & ~fr
    _count(f"rig {name} gather", differ, fr)
    agree = dev["gather_valid"] & r64["valid"] & r32["valid"] & ~fr
    _values_close(f"rig {name} gather rgb", dev["gather_rgb"], r64["rgb"], r32["rgb"], np.broadcast_to(agree[..., None], r64["rgb"].shape))
    assert (dev["gather_rgb"][~dev["gather_valid"]] == 0).all()
    assert not dev["gather_valid"][dev["gather_depth"] == 0].any()
    assert np.isfinite(dev["gather_depth"]).all() and (dev["gather_depth"] >= 0).all()


def test_missing_depth_never_becomes_a_value(on_device):
    r = rr.rig("A")
    dev, runs = on_device["A"]
    # the pixels of the pinhole depth image whose nearest raw sample is missing (same index in both runs): 0 and invalid
    r64, r32 = runs["gather"]
    idx = r64["index"]
    sure = (idx == r32["index"]) & (idx >= 0)
    for b in range(r.depth.shape[0]):
        missing = sure & ~rr._present(r.depth[b].reshape(-1)[np.clip(idx, 0, None)])
        if b == 0:
            assert missing.sum() >= 50  # the block of zeros
        assert (dev["gather_depth"][b][missing] == 0).all() and not dev["gather_valid"][b][missing].any()
    # an image of nothing but missing values: nothing lands anywhere
    bad = torch.tensor([0.0, float("nan"), float("inf"), float("-inf"), -1.0, -0.0]).repeat(r.depth[0].size // 6 + 1)[:r.depth[0].size]
    bad = bad.reshape(1, r.depth_cam.height, r.depth_cam.width).cuda()
    out = reg.depth_to_color(bad, r.depth_cam, _cuda(r.T_d2c[:1]), r.color_cam)
    assert (out == 0).all()
    gd, grgb, gvalid = reg.color_to_depth(bad, r.depth_cam, _cuda(r.T_d2c[:1]), _cuda(r.rgb[:1]), r.color_cam)
    assert (gd == 0).all() and (grgb == 0).all() and not gvalid.any()
    # a transform of NaN / inf / 1e30: in bounds, and nothing but zeros or positive finite values comes back
    for fill in (float("nan"), float("inf"), 1e30, -1e30):
        T = torch.full((1, 4, 4), fill).cuda()
        out = reg.depth_to_color(_cuda(r.depth[:1]), r.depth_cam, T, r.color_cam)
        gd, grgb, gvalid = reg.color_to_depth(_cuda(r.depth[:1]), r.depth_cam, T, _cuda(r.rgb[:1]), r.color_cam, zbuf=out, occlusion_tol=0.1)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all() and (out >= 0).all() and torch.isfinite(grgb).all()


def test_identity_rig():
    r = rr.rig("I")
    depth = r.depth.copy()
    depth[0, 3:9, 4:12] = 0.0
    depth[1, 10, 10] = np.nan
    depth[2, 7, 50] = -2.0
    depth[2, 8, 50] = np.inf
    # T = I exactly (inv(pose) @ pose, as the rig computes it, is the identity only up to rounding)
    eye = np.broadcast_to(np.eye(4, dtype=np.float32), r.T_d2c.shape).copy()
    assert np.abs(r.T_d2c - eye).max() < 1e-6
    d, rgb, T = _cuda(depth), _cuda(r.rgb), _cuda(eye)
    want = np.where(rr._present(depth), depth, np.float32(0))
    got = _np(reg.depth_to_color(d, r.depth_cam, T, r.color_cam))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "depth_to_color through the identity rig"
    assert (want > 0).mean() > 0.9
    # undistort: nearest is the identity for any intrinsics; bilinear where the pixel round trip is exact (EXACT_CAM)
    for img in (rgb, d):
        got = reg.undistort(img, r.depth_cam, reg.NEAREST)
        assert torch.equal(got.view(torch.int32), img.view(torch.int32)), "nearest undistort through the identity"
    for img in (rgb, torch.nan_to_num(d, nan=0.0, posinf=0.0)):
        got = reg.undistort(img, rr.EXACT_CAM, reg.BILINEAR)
        assert torch.equal(got.view(torch.int32), img.view(torch.int32)), "bilinear undistort through the identity"
    # color_to_depth: the rgb within the restatement's own gap
    gd, grgb, gvalid = reg.color_to_depth(d, r.depth_cam, T, rgb, r.color_cam)
    r64, r32 = (rr.color_to_depth(depth, r.depth_cam, eye, r.rgb, r.color_cam, dtype=dt) for dt in (np.float64, np.float32))
    assert np.array_equal(_np(gd).view(np.uint32), want.view(np.uint32))
    fr = rr.fragile("gather", r64, r32)
    _count("rig I gather", (_np(gvalid) != r64["valid"]) & ~fr, fr)
    agree = _np(gvalid) & r64["valid"] & r32["valid"] & ~fr
    _values_close("rig I gather rgb", _np(grgb), r64["rgb"], r32["rgb"], np.broadcast_to(agree[..., None], r64["rgb"].shape))


def test_two_calls_return_the_same_bytes():
    r = rr.rig("A")
    a, _ = _device(r)
    b, _ = _device(r)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def _analytic_color_views(r):
    """Per frame what the pinhole colour camera sees of the analytic scene: (depth [B,H,W], constant-surface mask [B,H,W])."""
    views = [rr.render(r.color_cam, p, raw=False) for p in r.pose_color]
    depth = np.stack([v[0] for v in views])
    # a depth pixel's footprint spans up to 3 colour pixels and is centred within 1 of its target: radius 3
    cs = np.stack([rr.constant_surface(v[1], 3) for v in views])
    return depth, cs & (depth > 0)


def test_to_color_against_the_analytic_scene(on_device):
    r = rr.rig("A")
    dev, runs = on_device["A"]
    out = reg.RgbdRig(r.depth_cam, r.color_cam).to_color(_cuda(r.depth), _cuda(r.rgb), _cuda(r.pose_depth), _cuda(r.pose_color))
    assert np.array_equal(_np(out.depth), dev["splat"]) and np.array_equal(_np(out.rgb), dev["undistort_rgb"])
    assert torch.equal(out.poses.cpu(), torch.from_numpy(r.pose_color)) and out.K.shape == (3, 3, 3)
    assert torch.equal(out.K[1].cpu(), r.color_cam.K())
    analytic, cs = _analytic_color_views(r)
    r64, r32 = runs["splat"]
    m = cs & (dev["splat"] > 0) & (r64["depth"] > 0) & (r32["depth"] > 0) & ~rr.fragile("splat", r64, r32)
    assert m.sum() > 0.4 * m.size
    rel = lambda d: np.abs(d.astype(np.float64)[m] - analytic[m]) / analytic[m]
    p99_dev, p99_ref = float(np.percentile(rel(dev["splat"]), 99)), float(np.percentile(rel(r64["depth"]), 99))
    gap = float((np.abs(r32["depth"].astype(np.float64) - r64["depth"])[m] / analytic[m]).max())
    print(f"rig A to_color: p99 relative depth error against the analytic scene on {int(m.sum())} constant-surface pixels: device "
          f"{p99_dev:.3e}, float64 restatement {p99_ref:.3e}; f32-vs-f64 gap {gap:.3e}")
    assert p99_dev <= p99_ref + gap


def test_occlusion_on_rig_c():
    r = rr.rig("C")
    dev_on, tol = _device(r)
    dev_off, _ = _device(r, zbuf_on=False)
    band, _ = rr.occluded_band(r, tol)
    assert band.sum() >= 150
    ref_on = rr.color_to_depth(r.depth, r.depth_cam, r.T_d2c, r.rgb, r.color_cam, zbuf=dev_on["splat"], occlusion_tol=tol)
    ref_off = rr.color_to_depth(r.depth, r.depth_cam, r.T_d2c, r.rgb, r.color_cam, zbuf=None)
    share_dev, share_ref = 1 - dev_on["gather_valid"][band].mean(), 1 - ref_on["valid"][band].mean()
    flagged = band & ~dev_on["gather_valid"]
    sphere = lambda rgb, m: (np.abs(rgb[m] - rr.BASE_COLORS[0]).max(-1) <= rr.COLOR_WAVE + 0.05).mean()
    valid_off_dev, valid_off_ref = dev_off["gather_valid"][flagged].mean(), ref_off["valid"][flagged].mean()
    col_dev, col_ref = sphere(dev_off["gather_rgb"], flagged), sphere(ref_off["rgb"], flagged)
    print(f"rig C: {int(band.sum())} band pixels, tol {tol:.4f} m: invalid with the test on: device {share_dev:.4f}, restatement "
          f"{share_ref:.4f}; of the flagged pixels, valid with the test off: {valid_off_dev:.4f} ({valid_off_ref:.4f}), carrying the "
          f"sphere's colour: {col_dev:.4f} ({col_ref:.4f})")
    assert share_dev >= share_ref and share_ref >= 0.9
    assert valid_off_dev >= valid_off_ref and valid_off_ref >= 0.9, "the occlusion test is what marks them"
    assert col_dev >= col_ref and col_ref >= 0.8
    # RgbdRig.to_depth: the same gather behind its own splat and its default tolerance
    out = reg.RgbdRig(r.depth_cam, r.color_cam).to_depth(_cuda(r.depth), _cuda(r.rgb), _cuda(r.pose_depth), _cuda(r.pose_color))
    assert np.array_equal(_np(out.valid), dev_on["gather_valid"]) and np.array_equal(_np(out.rgb), dev_on["gather_rgb"])
    assert np.array_equal(_np(out.depth), dev_on["gather_depth"], equal_nan=True)
    assert torch.equal(out.poses.cpu(), torch.from_numpy(r.pose_depth)) and torch.equal(out.K[0].cpu(), r.depth_cam.K())


class _ReplayClip:
    """A backbone stand-in: one seeded feature map per frame, whatever the image."""

    def __init__(self, dim, n, npy, npx):
        self.feature_dim = dim
        self.maps = torch.randn((n, dim, npy, npx), generator=torch.Generator().manual_seed(5)).cuda()

    def img_inference_tiled(self, rgb, patch_size, patch_stride):
        return self.maps[: rgb.shape[0]]


def test_registered_frames_go_into_the_fusion():
    from spatially_aware_ai_amd import ClipFusion

    r = rr.rig("A8")
    n, dim = r.depth.shape[0], 64
    grid = syn.make_grid(48)
    vs = grid.voxel_size
    cam = r.color_cam.pinhole()
    npy, npx = syn.feature_map_shape(cam.width, cam.height)

    def volume():
        return ClipFusion(grid.origin, grid.voxel_size, grid.nvox, grid.trunc, False, _ReplayClip(dim, n, npy, npx), None, 10, 10,
                          keep_xyz_world=False).cuda()

    rig = reg.RgbdRig(r.depth_cam, r.color_cam)
    frames = rig.to_color(_cuda(r.depth), _cuda(r.rgb), _cuda(r.pose_depth), _cuda(r.pose_color))
    fused = volume()
    fused.integrate(frames.depth, frames.rgb, frames.poses, frames.K)  # straight in: no copies in between
    analytic, cs = _analytic_color_views(r)
    ideal = volume()
    ideal_rgb = np.stack([rr.render(r.color_cam, p, raw=False)[2] for p in r.pose_color])
    ideal.integrate(_cuda(analytic), _cuda(ideal_rgb), frames.poses, frames.K)
    view = 2
    got, base = (_np(v.render(frames.poses[view], frames.K[view], cam.height, cam.width).depth) for v in (fused, ideal))
    m = cs[view] & (got > 0) & (base > 0)
    assert m.sum() > 0.3 * m.size
    p99 = lambda d: float(np.percentile(np.abs(d[m] - analytic[view][m]) / vs, 99))
    # the float64 restatement's registration error on the frames that were fused, in voxels (a depth error moves the surface by
    # at most as much)
    r64 = rr.depth_to_color(r.depth, r.depth_cam, r.T_d2c, r.color_cam, dtype=np.float64)["depth"]
    mr = cs & (r64 > 0)
    reg_err = float(np.percentile(np.abs(r64[mr] - analytic[mr]) / vs, 99))
    print(f"fused from registered frames: p99 |rendered - analytic| = {p99(got):.4f} voxels; from ideal frames {p99(base):.4f}; the "
          f"float64 restatement's p99 registration error {reg_err:.4f} voxels ({int(m.sum())} pixels)")
    assert p99(got) <= p99(base) + reg_err
    # the other direction is accepted as it comes (shape, dtype, contiguity)
    back = rig.to_depth(_cuda(r.depth), _cuda(r.rgb), _cuda(r.pose_depth), _cuda(r.pose_color))
    for t in (back.depth, back.rgb, back.poses, back.K):
        assert t.is_contiguous() and t.dtype == torch.float32 and t.is_cuda
    npy, npx = syn.feature_map_shape(r.depth_cam.width, r.depth_cam.height)
    other = ClipFusion(grid.origin, grid.voxel_size, grid.nvox, grid.trunc, False, _ReplayClip(dim, n, npy, npx), None, 10, 10,
                       keep_xyz_world=False).cuda()
    other.integrate(back.depth, back.rgb, back.poses, back.K)
    assert int((other.weight > 0).sum()) > 1000
