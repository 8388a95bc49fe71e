"""Free-space carving (not in the reference): fused voxels that later frames see THROUGH are taken out of the volume
again -- ``observe_free_space`` and ``carve`` as a mixin of ``clipfusion._FusionVolumeMixin``, what they return, and the host-side
preparation of the depth (``erode_depth``).  ``clipfusion`` re-exports these names; nothing here imports ``clipfusion``."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from . import _abi
from ._lib import SafError, check, lib, require_cuda


@dataclass
class FreeSpaceEvidence:
    """What ``observe_free_space`` returns and ``carve`` takes: per voxel of the box (``index_offset``, ``nvox`` on the module's
    lattice) two int32 DEVICE tensors [N] -- ``seen``: the frames that looked through the voxel (sdf > 1), ``hit``: the frames that
    support a surface there (|sdf| <= 1); both stay 0 where ``weight == 0`` -- and ``n_frames``, the frames observed so far."""

    seen: torch.Tensor
    hit: torch.Tensor
    n_frames: int
    index_offset: tuple
    nvox: tuple


@dataclass
class CarveResult:
    """What ``carve`` returns.  The four counters are 0-d int64 DEVICE tensors -- reading one synchronises: voxels with
    ``weight > 0`` before the call, voxels carved, voxels kept because more than ``max_support`` frames support them although
    ``min_views`` or more look through, and voxels kept because fewer than ``min_views`` (but at least one) look through.
    ``mask``: bool [N] on the device, True where a voxel was carved (``return_mask=True``), else None.  ``evidence``: what the
    decision was taken on."""

    n_touched: torch.Tensor
    n_carved: torch.Tensor
    n_supported: torch.Tensor
    n_few_views: torch.Tensor
    mask: torch.Tensor | None
    evidence: FreeSpaceEvidence
    min_views: int
    max_support: int


def erode_depth(depth_imgs, erode=1):
    """The depth images [B,H,W] as the carve looks at them.  ``erode == 0``: unchanged.  ``erode == e >= 1``: a pixel becomes the
    MINIMUM over its (2e+1) x (2e+1) window, clipped at the image border, if every pixel of that clipped window is finite and
    > 0; otherwise it becomes 0 (missing).  A voxel on an object's silhouette projects onto an edge pixel, and a pose error of a
    pixel lets the background "see through" the rim: the minimum is the conservative depth, and a window with a hole in it
    claims nothing.  Torch, on whatever device the images are; selections only, so the values are exact."""
    if isinstance(erode, bool) or not isinstance(erode, int) or erode < 0:
        raise SafError(f"erode must be an int >= 0, got {erode!r}")
    if erode == 0:
        return depth_imgs
    d = depth_imgs.to(torch.float32)
    ok = torch.isfinite(d) & (d > 0)
    inf = torch.full_like(d, float("inf"))
    k = 2 * erode + 1
    # (max_pool2d pads with -inf: the padding never wins, which is the window clipped at the border)
    low = -F.max_pool2d(-torch.where(ok, d, inf)[:, None], k, stride=1, padding=erode)[:, 0]
    bad = F.max_pool2d((~ok).to(torch.float32)[:, None], k, stride=1, padding=erode)[:, 0] > 0
    return torch.where(bad, torch.zeros_like(d), low)


def _count_arg(name, value, least):
    if isinstance(value, bool) or not isinstance(value, int) or value < least:
        raise SafError(f"carve: {name} must be an int >= {least}, got {value!r}")
    return value


class _CarveMixin:
    """``observe_free_space`` and ``carve`` of a fusion module, on ``_FusionVolumeMixin``'s buffers, queue and ``_c_volume``."""

    def _carve_refusals(self, call):
        self._refuse_unfit(call, "first")
        if self.accum_mode != _abi.SAF_RUNNING_MEAN:
            raise SafError(f"{call}: running means only: a SAF_SUM volume belongs to the multi-rank job, whose merge adds its sums")

    def _box(self):
        return tuple(int(v) for v in self.index_offset), tuple(int(v) for v in self.nvox)

    def _check_evidence(self, call, evidence):
        if not isinstance(evidence, FreeSpaceEvidence):
            raise SafError(f"{call}: evidence must be a FreeSpaceEvidence, got {type(evidence).__name__}")
        off, nvox = self._box()
        if (tuple(evidence.index_offset), tuple(evidence.nvox)) != (off, nvox):
            raise SafError(f"{call}: the evidence belongs to the box {tuple(evidence.nvox)} at {tuple(evidence.index_offset)}, the module "
                           f"holds {nvox} at {off} now (move_grid, coarsen and resample change the box: observe again)")
        n = nvox[0] * nvox[1] * nvox[2]
        for name in ("seen", "hit"):
            t = getattr(evidence, name)
            if not torch.is_tensor(t) or t.dtype != torch.int32 or t.numel() != n or not t.is_contiguous():
                raise SafError(f"{call}: evidence.{name} must be a contiguous int32 tensor of {n} entries")

    def _quiet_queue(self):
        """The frames still queued behind ``integrate()`` are fused and the current stream waits for them.  A deferred clear stays
        owed: neither pass reads the row of a weight-0 voxel, and a carved voxel's row is written zero."""
        self._flush_pending(final=True)
        self.__dict__["_queue"].wait(self)

    def observe_free_space(self, depth_imgs, poses, K, erode=1, evidence=None):
        """Gather, for every touched voxel (``weight > 0``), what the frames ``depth_imgs`` [B,H,W] / ``poses`` [B,4,4] / ``K``
        [B,3,3] say about the space it stands in: ``seen`` counts the frames that look THROUGH the voxel -- the frame's depth tap at
        the voxel's projection lies more than ``trunc`` behind it: ``tsdf_valid and not valid`` of the reference's ``integrate``
        (clipfusion.py:669-679) -- and ``hit`` the frames that support a surface there (``valid``); the decisions are the fuse
        path's own (saf_free_space_observe, include/saf.h).  Needs depth, pose and K only: no frame goes through a
        backbone.  ``erode``: ``erode_depth`` is applied to the depth first (default 1: the 3 x 3 minimum, 0 where the window has
        a hole).  ``evidence``: counts of earlier calls to ADD to (frames may come in any split and order); None: zeroed counts.

        Frames still queued behind ``integrate()`` are fused first; a deferred clear stays owed; the volume is only read.
        Returns the ``FreeSpaceEvidence``; nothing is read back.  ``SafError`` for a module built with ``x_planes``, one that holds
        only reduce-scattered stripes, a poisoned one, a ``SAF_SUM`` volume, inputs of other shapes than the above, and an
        ``evidence`` whose box is not the module's current one."""
        self._carve_refusals("observe_free_space")
        if evidence is not None:
            self._check_evidence("observe_free_space", evidence)
        if not torch.is_tensor(depth_imgs) or depth_imgs.dim() != 3 or depth_imgs.shape[0] < 1:
            raise SafError("observe_free_space: depth_imgs must be a [B,H,W] tensor with B >= 1")
        b = int(depth_imgs.shape[0])
        if not torch.is_tensor(poses) or tuple(poses.shape) != (b, 4, 4) or not torch.is_tensor(K) or tuple(K.shape) != (b, 3, 3):
            raise SafError(f"observe_free_space: poses must be [{b},4,4] and K [{b},3,3]")
        bufs = self._buffers
        require_cuda(bufs["weight"], "the fusion volume")
        dev = bufs["weight"].device
        self._quiet_queue()
        vol = self._c_volume(for_fuse=True)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
            depth, poses_d, k_d = erode_depth(f32(depth_imgs), erode).contiguous(), f32(poses), f32(K)
            if evidence is None:
                off, nvox = self._box()
                n = nvox[0] * nvox[1] * nvox[2]
                evidence = FreeSpaceEvidence(torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                                             0, off, nvox)
            elif evidence.seen.device != dev or evidence.hit.device != dev:
                raise SafError(f"observe_free_space: the evidence is not on the volume's device ({dev})")
            check(lib().saf_free_space_observe(C.byref(vol), _abi.ptr(depth), b, int(depth.shape[1]), int(depth.shape[2]),
                                               _abi.ptr(poses_d), _abi.ptr(k_d), _abi.ptr(evidence.seen), _abi.ptr(evidence.hit),
                                               stream.cuda_stream), "saf_free_space_observe")
            for t in (depth, poses_d, k_d):
                t.record_stream(stream)  # (the launch is asynchronous)
        evidence.n_frames += b
        return evidence

    def carve(self, evidence=None, depth_imgs=None, poses=None, K=None, min_views=2, max_support=0, erode=1, return_mask=False):
        """Take out of the volume what later frames see through: a voxel is CARVED iff ``weight > 0``, at least ``min_views`` frames
        of the evidence look through it (``seen >= min_views``) and at most ``max_support`` support a surface there
        (``hit <= max_support``).  A carved voxel becomes the voxel a fresh module holds -- ``weight``, ``tsdf_weight``, ``tsdf``,
        ``rgb``, its feature row and its label histogram are zero bytes -- so that fusing the new frames afterwards gives, on the
        carved voxels, exactly what a fresh volume would hold; every other byte of the volume stays (saf_volume_carve,
        include/saf.h).  Either ``evidence`` (``observe_free_space``'s) or the frames ``depth_imgs`` / ``poses`` / ``K``
        (observed here, ``erode`` as there; with both, the frames are added to the evidence first).

        ``min_views`` and ``erode`` are the robustness knobs: there is no margin beyond ``trunc``, and WHEN to carve is the
        caller's decision.  Frames that were fused into carved voxels can no longer be taken out: ``deintegrate`` skips and counts
        such a voxel, as it does for any voxel whose count is 0.  ``voxel_obj_idx`` and ``objects_segmentation_color`` describe a
        labelling the volume no longer has and are deleted.  Frames still queued behind ``integrate()`` are fused first; a deferred
        clear stays owed.  Returns a ``CarveResult``; its counters are device tensors, nothing is read back here.  ``SafError``,
        with the volume unchanged, for what ``observe_free_space`` refuses, ``min_views < 1``, ``max_support < 0`` and neither
        evidence nor frames."""
        self._carve_refusals("carve")
        min_views, max_support = _count_arg("min_views", min_views, 1), _count_arg("max_support", max_support, 0)
        frames = (depth_imgs, poses, K)
        if any(t is not None for t in frames) and not all(t is not None for t in frames):
            raise SafError("carve: depth_imgs, poses and K come together")
        if evidence is None and depth_imgs is None:
            raise SafError("carve: give the evidence of observe_free_space, or frames (depth_imgs, poses, K)")
        if evidence is not None:
            self._check_evidence("carve", evidence)
        if depth_imgs is not None:
            evidence = self.observe_free_space(depth_imgs, poses, K, erode=erode, evidence=evidence)
        bufs = self._buffers
        require_cuda(bufs["weight"], "the fusion volume")
        dev = bufs["weight"].device
        if evidence.seen.device != dev or evidence.hit.device != dev:
            raise SafError(f"carve: the evidence is not on the volume's device ({dev})")
        self._quiet_queue()
        vol = self._c_volume(for_fuse=True)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            counts = torch.zeros(4, dtype=torch.int64, device=dev)
            mask = torch.empty(evidence.seen.numel(), dtype=torch.uint8, device=dev) if return_mask else None
            check(lib().saf_volume_carve(C.byref(vol), _abi.ptr(evidence.seen), _abi.ptr(evidence.hit), min_views, max_support,
                                         _abi.ptr(mask), _abi.ptr(counts), stream.cuda_stream), "saf_volume_carve")
        self.__dict__["_shard16"] = None
        self._drop_labelling()
        return CarveResult(n_touched=counts[0], n_carved=counts[1], n_supported=counts[2], n_few_views=counts[3],
                           mask=None if mask is None else mask.bool(), evidence=evidence, min_views=min_views, max_support=max_support)
