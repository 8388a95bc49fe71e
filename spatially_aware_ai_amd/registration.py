"""The rig front-end: a headset's depth and colour cameras registered on the device before fusion.

A Magic Leap 2 frame (what the reference's ``magicleap2_camera_match.py`` prepares) has a depth image and a colour image from
two cameras with different resolutions, intrinsics, 5-coefficient lens distortions and poses; ``integrate()``, ``saf_frame`` and
``backproject_pcd`` assume one pinhole ``K`` and one pose for everything in a frame.  ``RgbdRig`` takes a batch of such frames to
exactly what ``integrate()`` consumes, in HIP (include/saf.h, "Rig front-end"; csrc/saf_register.hip): lens undistortion,
depth -> colour registration (a z-buffered splat) and colour -> depth registration (a gather with an occlusion test).

Not mirrored from the reference script: its arithmetic (a per-pixel Python loop behind two ``cv2.undistort`` calls, without an
occlusion test, ending in ``breakpoint()``) and its relative-pose lines, which are dubious; the relative pose here is
``inv(pose_color) @ pose_depth`` for camera -> world poses.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, replace

import torch

from . import _abi
from ._lib import check, current_stream_ptr, lib, require_cuda

NEAREST, BILINEAR = 0, 1


@dataclass(frozen=True)
class CameraModel:
    """A camera of the rig: image size, pinhole intrinsics (no skew) and ``dist = (k1, k2, p1, p2, k3)`` in OpenCV's order."""

    width: int
    height: int
    fx: float
    fy: float
    cx: float
    cy: float
    dist: tuple = (0.0,) * 5

    def __post_init__(self):
        if len(tuple(self.dist)) != 5:
            raise ValueError("dist holds five coefficients: k1, k2, p1, p2, k3")
        object.__setattr__(self, "dist", tuple(float(d) for d in self.dist))

    def K(self) -> torch.Tensor:
        """[3,3] f32 intrinsics."""
        return torch.tensor([[self.fx, 0.0, self.cx], [0.0, self.fy, self.cy], [0.0, 0.0, 1.0]], dtype=torch.float32)

    def pinhole(self) -> "CameraModel":
        """The same camera without lens distortion."""
        return replace(self, dist=(0.0,) * 5)

    def scaled(self, width: int, height: int) -> "CameraModel":
        """The same view at another resolution: fx, cx scale with the width, fy, cy with the height (pixel centres at
        integers, as everywhere in this package: u' = s u)."""
        sx, sy = width / self.width, height / self.height
        return replace(self, width=int(width), height=int(height), fx=self.fx * sx, fy=self.fy * sy, cx=self.cx * sx, cy=self.cy * sy)

    def _c(self) -> _abi.SafCamera:
        return _abi.SafCamera(int(self.width), int(self.height), self.fx, self.fy, self.cx, self.cy, (C.c_float * 5)(*self.dist))


def camera_from_meta(meta) -> CameraModel:
    """The camera of one of the headset's per-frame JSON objects, already parsed (``json.load``): ``intrinsics.Width``,
    ``.Height``, ``.FocalLength.x/y``, ``.PrincipalPoint.x/y`` and ``.Distortion`` (five numbers, taken as k1, k2, p1, p2, k3).
    Only the layout is read: no EXR or image decoding, and no change of axis conventions."""
    i = meta["intrinsics"]
    dist = tuple(float(d) for d in i["Distortion"])
    if len(dist) != 5:
        raise ValueError(f"intrinsics.Distortion holds {len(dist)} numbers, not 5")
    return CameraModel(int(i["Width"]), int(i["Height"]), float(i["FocalLength"]["x"]), float(i["FocalLength"]["y"]),
                       float(i["PrincipalPoint"]["x"]), float(i["PrincipalPoint"]["y"]), dist)


def pose_from_meta(meta) -> torch.Tensor:
    """[4,4] f64 from ``pose.e00 .. pose.e33`` (row-major) of the same object, as recorded: no change of axis conventions."""
    p = meta["pose"]
    return torch.tensor([[float(p[f"e{r}{c}"]) for c in range(4)] for r in range(4)], dtype=torch.float64)


def _images(t, name, shape_tail):
    """A contiguous f32 [B, ...] tensor on the HIP device (what the loaders yield; anything else is converted once)."""
    t = torch.as_tensor(t)
    require_cuda(t, name)
    if t.dim() != 1 + len(shape_tail) or any(s is not None and int(t.shape[1 + i]) != s for i, s in enumerate(shape_tail)):
        raise ValueError(f"{name} must be [B, {', '.join('C' if s is None else str(s) for s in shape_tail)}], not {tuple(t.shape)}")
    if t.shape[0] < 1:
        raise ValueError(f"{name} is an empty batch")
    return t.to(torch.float32).contiguous()


def _transforms(T_d2c, batch, dev):
    T = torch.as_tensor(T_d2c)
    if T.dim() == 2:
        T = T[None].expand(batch, 4, 4)
    if tuple(T.shape) != (batch, 4, 4):
        raise ValueError(f"T_d2c must be [4,4] or [{batch},4,4], not {tuple(T.shape)}")
    return T.to(device=dev, dtype=torch.float32).contiguous()


def undistort(images, cam: CameraModel, interp=BILINEAR, out_cam: CameraModel | None = None):
    """``images`` [B,H,W,C] or [B,H,W] (f32, on the HIP device) as the pinhole ``out_cam`` (default ``cam.pinhole()``) sees them
    (saf_undistort_images).  ``interp``: ``BILINEAR`` for colour, ``NEAREST`` for depth and label maps -- bilinear invents
    surfaces across depth edges."""
    images = torch.as_tensor(images)
    flat = images.dim() == 3
    src = _images(images[..., None] if flat else images, "images", (cam.height, cam.width, None))
    out_cam = cam.pinhole() if out_cam is None else out_cam
    b, ch = int(src.shape[0]), int(src.shape[3])
    dst = torch.empty((b, out_cam.height, out_cam.width, ch), dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        rc = lib().saf_undistort_images(src.data_ptr(), b, ch, C.byref(cam._c()), C.byref(out_cam._c()), int(interp), dst.data_ptr(),
                                        current_stream_ptr())
    check(rc, "saf_undistort_images")
    return dst[..., 0] if flat else dst


def depth_to_color(depth, depth_cam: CameraModel, T_d2c, color_cam: CameraModel, max_footprint=8):
    """Raw ``depth`` [B,Hd,Wd] splatted into the pinhole of ``color_cam``: [B,Hc,Wc] camera z, 0 where nothing lands
    (saf_depth_to_color).  ``T_d2c`` [B,4,4] or [4,4]: depth-camera -> colour-camera coordinates."""
    d = _images(depth, "depth", (depth_cam.height, depth_cam.width))
    b = int(d.shape[0])
    T = _transforms(T_d2c, b, d.device)
    out = torch.empty((b, color_cam.height, color_cam.width), dtype=torch.float32, device=d.device)
    with torch.cuda.device(d.device):
        rc = lib().saf_depth_to_color(d.data_ptr(), C.byref(depth_cam._c()), T.data_ptr(), b, C.byref(color_cam._c()),
                                      int(max_footprint), out.data_ptr(), None, 0, current_stream_ptr())
    check(rc, "saf_depth_to_color")
    return out


def color_to_depth(depth, depth_cam: CameraModel, T_d2c, color, color_cam: CameraModel, zbuf=None, zbuf_cam=None,
                   occlusion_tol=0.0, out_cam: CameraModel | None = None):
    """Per pixel of the pinhole ``out_cam`` (default ``depth_cam.pinhole()``): ``(depth [B,H,W], rgb [B,H,W,3], valid [B,H,W]
    bool)`` -- the undistorted depth (nearest) and the colour the colour camera saw of that point (saf_color_to_depth).
    ``zbuf``: a ``depth_to_color`` result for the pinhole ``zbuf_cam`` (default ``color_cam``); a point more than
    ``occlusion_tol`` metres behind it is invalid.  ``zbuf=None``: no occlusion test."""
    d = _images(depth, "depth", (depth_cam.height, depth_cam.width))
    col = _images(color, "color", (color_cam.height, color_cam.width, 3))
    b = int(d.shape[0])
    if col.shape[0] != b or col.device != d.device:
        raise ValueError("depth and color must hold the same frames on the same device")
    T = _transforms(T_d2c, b, d.device)
    out_cam = depth_cam.pinhole() if out_cam is None else out_cam
    zcam = None
    if zbuf is not None:
        zcam = color_cam if zbuf_cam is None else zbuf_cam
        zbuf = _images(zbuf, "zbuf", (zcam.height, zcam.width))
        if zbuf.shape[0] != b or zbuf.device != d.device:
            raise ValueError("zbuf must hold the same frames on the same device")
    shape = (b, out_cam.height, out_cam.width)
    out_d = torch.empty(shape, dtype=torch.float32, device=d.device)
    out_rgb = torch.empty(shape + (3,), dtype=torch.float32, device=d.device)
    out_valid = torch.empty(shape, dtype=torch.uint8, device=d.device)
    with torch.cuda.device(d.device):
        rc = lib().saf_color_to_depth(d.data_ptr(), C.byref(depth_cam._c()), C.byref(out_cam._c()), T.data_ptr(), b, col.data_ptr(),
                                      C.byref(color_cam._c()), None if zbuf is None else zbuf.data_ptr(),
                                      None if zcam is None else C.byref(zcam._c()), float(occlusion_tol), out_d.data_ptr(),
                                      out_rgb.data_ptr(), out_valid.data_ptr(), current_stream_ptr())
    check(rc, "saf_color_to_depth")
    return out_d, out_rgb, out_valid.bool()


def relative_pose(pose_depth, pose_color) -> torch.Tensor:
    """``T_d2c = inv(pose_color) @ pose_depth`` [B,4,4] for camera -> world poses (the convention of ``saf_frame.pose``), in
    float64 on the host, rounded once to f32."""
    pd = torch.as_tensor(pose_depth).detach().cpu().double().reshape(-1, 4, 4)
    pc = torch.as_tensor(pose_color).detach().cpu().double().reshape(-1, 4, 4)
    if pd.shape != pc.shape:
        raise ValueError("one depth pose and one colour pose per frame")
    return (torch.linalg.inv(pc) @ pd).float()


@dataclass
class RegisteredFrames:
    """What ``integrate(depth, rgb, poses, K)`` consumes, on the device: depth [B,H,W], rgb [B,H,W,3], poses [B,4,4] (camera ->
    world), K [B,3,3]; ``valid`` [B,H,W] bool where the direction produces one (``to_depth``)."""

    depth: torch.Tensor
    rgb: torch.Tensor
    poses: torch.Tensor
    K: torch.Tensor
    valid: torch.Tensor | None = None


class RgbdRig:
    """A depth camera and a colour camera on one headset.

    ``max_footprint``: the largest size, in colour pixels, a depth pixel is splatted to.  ``occlusion_tol``: metres; ``None``
    takes 2 % of the median depth the colour camera sees in the batch, per call (the kernel takes one scalar) -- an UNMEASURED default: no capture of
    a real headset was at hand to tune it on.

    ``to_color`` is the direction the fused path wants: the CLIP and panoptic backbones see the true colour image at its own
    resolution, and only depth is resampled.  ``to_depth`` is the reference script's direction.  In both the relative pose is
    ``inv(pose_color) @ pose_depth`` (poses are camera -> world, as ``saf_frame.pose``), computed in float64 on the host and
    rounded once to f32; the reference script's own relative-pose lines are not mirrored.  The outputs go straight into
    ``ClipFusion.integrate`` / ``ClipSeemFusion.integrate`` / ``backproject_pcd``: no copies in between."""

    def __init__(self, depth_cam: CameraModel, color_cam: CameraModel, max_footprint=8, occlusion_tol=None):
        if not 1 <= int(max_footprint) <= 16:
            raise ValueError("max_footprint is 1 .. 16 colour pixels")
        self.depth_cam, self.color_cam = depth_cam, color_cam
        self.max_footprint = int(max_footprint)
        self.occlusion_tol = occlusion_tol

    def _poses(self, pose, batch, dev):
        p = torch.as_tensor(pose).reshape(-1, 4, 4)
        if p.shape[0] != batch:
            raise ValueError(f"{batch} frames need {batch} poses, not {p.shape[0]}")
        return p.to(device=dev, dtype=torch.float32).contiguous()

    def to_color(self, depth, rgb, pose_depth, pose_color) -> RegisteredFrames:
        """Raw ``depth`` [B,Hd,Wd] and raw ``rgb`` [B,Hc,Wc,3] -> frames in the undistorted colour camera: depth splatted, rgb
        undistorted bilinearly, ``poses = pose_color``, ``K = color_cam.pinhole().K()``."""
        T = relative_pose(pose_depth, pose_color)
        d = depth_to_color(depth, self.depth_cam, T, self.color_cam, self.max_footprint)
        c = undistort(rgb, self.color_cam, BILINEAR)
        b = int(d.shape[0])
        return RegisteredFrames(d, c, self._poses(pose_color, b, d.device), self.color_cam.K().to(d.device).expand(b, 3, 3).contiguous())

    def to_depth(self, depth, rgb, pose_depth, pose_color) -> RegisteredFrames:
        """The same inputs -> frames in the undistorted depth camera: depth undistorted (nearest), rgb gathered from the raw
        colour image with the occlusion test against a splat computed here, ``valid``, ``poses = pose_depth``, the depth
        pinhole's ``K``."""
        T = relative_pose(pose_depth, pose_color)
        zbuf = depth_to_color(depth, self.depth_cam, T, self.color_cam, self.max_footprint)
        tol = self.occlusion_tol
        if tol is None:
            seen = zbuf[zbuf > 0]
            tol = 0.02 * float(seen.median()) if seen.numel() else 0.0
        d, c, valid = color_to_depth(depth, self.depth_cam, T, rgb, self.color_cam, zbuf=zbuf, occlusion_tol=tol)
        b = int(d.shape[0])
        return RegisteredFrames(d, c, self._poses(pose_depth, b, d.device), self.depth_cam.K().to(d.device).expand(b, 3, 3).contiguous(),
                                valid)
