"""A fused volume taken to another box or lattice and kept fusing (not in the reference): ``move_grid``, ``absorb``
(4.20), ``coarsen`` (4.21) and ``resample`` (4.22) as a mixin of ``clipfusion._FusionVolumeMixin``, what they return, the host
arithmetic of boxes and lattices, and the steps the four share, once each.  ``clipfusion`` re-exports these names; nothing here imports ``clipfusion``."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _abi
from ._lib import SafError, check, lib, require_cuda

_DT = {torch.float32: _abi.SAF_F32, torch.bfloat16: _abi.SAF_BF16, torch.float16: _abi.SAF_F16}


def _axis_tables(origin, voxel_size, nvox, index_offset=(0, 0, 0), x_planes=None):
    """Per-axis voxel-centre coordinates, element for element what the reference computes as
    ``xyz_idx * voxel_size + origin`` (clipfusion.py:617-622): int64 index * python float -> f32
    product, + f32 origin.  ``index_offset``: the module holds the sub-grid that starts at this voxel index of the grid
    anchored at ``origin`` (a slab of a voxel-sharded volume): the same expression on the same indices, bit for bit.
    ``x_planes``: the x indices the module holds, in its own order (a slab made of several blocks of x-planes)."""
    origin = torch.as_tensor(origin).detach().cpu()
    idx = [torch.arange(int(nvox[a])) + int(index_offset[a]) for a in range(3)]
    if x_planes is not None:
        idx[0] = torch.as_tensor(x_planes, dtype=torch.int64).detach().cpu()
        if idx[0].dim() != 1 or idx[0].numel() != int(nvox[0]):
            raise ValueError("x_planes must list nvox[0] x indices")
        # The windowed path classifies 4 x 4 x 16 bricks against a bounding sphere built from a brick's first and last
        # x-plane: every group of 4 consecutive entries must be 4 consecutive planes (a rank's slab is made of whole blocks).
        if int(nvox[0]) % 4 == 0:
            q = idx[0].view(-1, 4)
            if not bool((q[:, 1:] - q[:, :-1] == 1).all()):
                raise ValueError("x_planes must consist of runs of 4 consecutive x indices (blocks of slab_planes_of_rank)")
    return [(idx[a] * voxel_size + origin[a]).to(torch.float32).contiguous() for a in range(3)]


def _xyz_world(ax, nvox):
    """The reference's ``xyz_world`` [N,3] (clipfusion.py:617-622) from the three axis tables."""
    nx, ny, nz = (int(v) for v in nvox)
    return torch.stack(
        (
            ax[0][:, None, None].expand(nx, ny, nz),
            ax[1][None, :, None].expand(nx, ny, nz),
            ax[2][None, None, :].expand(nx, ny, nz),
        ),
        dim=-1,
    ).reshape(-1, 3)


def _volume_struct(bufs, ax, nvox, feat_dim, accum_mode, trunc):
    """The ``saf_volume`` descriptor (include/saf.h) of the buffers ``bufs`` and the axis tables ``ax``."""
    p = _abi.ptr
    labels = bufs.get("labels_one_hot")
    return _abi.SafVolume(
        int(nvox[0]), int(nvox[1]), int(nvox[2]), int(feat_dim), 0 if labels is None else int(labels.shape[1]),
        _DT[bufs["clip_feat"].dtype], int(accum_mode), float(trunc), p(ax[0]), p(ax[1]), p(ax[2]),
        p(bufs["tsdf"]), p(bufs["tsdf_weight"]), p(bufs["weight"]), p(bufs["rgb"]), p(bufs["clip_feat"]), p(labels))


def _box_overlap(off_a, n_a, off_b, n_b):
    """The voxels two boxes of one lattice share: (extent, low corner in a's own indices, low corner in b's); three times
    (0, 0, 0) when they share none."""
    lo = tuple(max(off_a[k], off_b[k]) for k in range(3))
    hi = tuple(min(off_a[k] + n_a[k], off_b[k] + n_b[k]) for k in range(3))
    if not all(hi[k] > lo[k] for k in range(3)):
        return (0, 0, 0), (0, 0, 0), (0, 0, 0)
    return tuple(hi[k] - lo[k] for k in range(3)), tuple(lo[k] - off_a[k] for k in range(3)), tuple(lo[k] - off_b[k] for k in range(3))


@dataclass
class GridMove:
    """What ``move_grid`` returns.  Boxes are (index offset on the module's lattice, voxels per axis); the overlap is given by its
    size and by its low corner in the old and in the new box's own indices (all zeros when the boxes share no voxel).  The four
    counters are 0-d int64 DEVICE tensors -- reading one synchronises: feature rows (voxels with ``weight > 0``) and TSDF voxels
    (``tsdf_weight > 0``) that the new box took over, and those of the old box that it left behind."""

    old_index_offset: tuple
    old_nvox: tuple
    index_offset: tuple
    nvox: tuple
    overlap_nvox: tuple
    overlap_in_old: tuple
    overlap_in_new: tuple
    rows_carried: torch.Tensor
    rows_dropped: torch.Tensor
    tsdf_carried: torch.Tensor
    tsdf_dropped: torch.Tensor


@dataclass
class GridAbsorb:
    """What ``absorb`` returns.  Boxes are (index offset on the shared lattice, voxels per axis): this module's after the call and
    the other's; the overlap is given by its size and by its low corner in each box's own indices (all zeros when the boxes share no
    voxel); ``move`` is the ``GridMove`` of the growth, or None.  The counters are 0-d int64 DEVICE tensors -- reading one
    synchronises: feature rows (``weight > 0`` in the other volume) and TSDF voxels (``tsdf_weight > 0``) that were blended with
    what was here, that were copied into empty voxels, and that lie outside this module's final box and were not taken in."""

    index_offset: tuple
    nvox: tuple
    other_index_offset: tuple
    other_nvox: tuple
    overlap_nvox: tuple
    overlap_in_self: tuple
    overlap_in_other: tuple
    move: GridMove | None
    rows_blended: torch.Tensor
    rows_copied: torch.Tensor
    tsdf_blended: torch.Tensor
    tsdf_copied: torch.Tensor
    rows_outside: torch.Tensor
    tsdf_outside: torch.Tensor


@dataclass
class GridCoarsen:
    """What ``coarsen`` returns: the factor, and the lattice and box (``origin``, ``voxel_size``, index offset, voxels per axis)
    before and after.  The four counters are 0-d int64 DEVICE tensors -- reading one synchronises: coarse voxels whose feature row
    (TSDF value) is the blend of two or more fine voxels, and those that are the copy of a single one."""

    factor: int
    old_origin: object
    old_voxel_size: float
    old_index_offset: tuple
    old_nvox: tuple
    origin: object
    voxel_size: float
    index_offset: tuple
    nvox: tuple
    rows_blended: torch.Tensor
    rows_copied: torch.Tensor
    tsdf_blended: torch.Tensor
    tsdf_copied: torch.Tensor


@dataclass
class GridResample:
    """What ``resample`` returns: the lattice and box (``origin``, ``voxel_size``, index offset, voxels per axis) before and after,
    the ``transform`` (4 x 4 float64 ``new_from_old``), the ``matrix`` ([3, 4] float32: a new voxel's local index to a continuous
    local index of the old box, what the pass was given) and ``min_cover``.  The four counters are 0-d int64 DEVICE tensors --
    reading one synchronises: new voxels whose feature row (TSDF value) is the blend of two or more old voxels, and those that
    are the copy of a single one."""

    old_origin: object
    old_voxel_size: float
    old_index_offset: tuple
    old_nvox: tuple
    origin: object
    voxel_size: float
    index_offset: tuple
    nvox: tuple
    transform: np.ndarray
    matrix: np.ndarray
    min_cover: float
    rows_blended: torch.Tensor
    rows_copied: torch.Tensor
    tsdf_blended: torch.Tensor
    tsdf_copied: torch.Tensor


class _GridOpsMixin:
    """``move_grid``, ``absorb``, ``coarsen`` and ``resample`` of a fusion module, on ``_FusionVolumeMixin``'s buffers, queue and ``_c_volume``."""

    def _refuse_unfit(self, call, before, who="this", pair=False):
        """``SafError`` for a module built with ``x_planes``, holding only stripes, or poisoned.  ``pair``: one of two, named ``who``."""
        if self.x_planes is not None:
            raise SafError(f"{call}() needs {'boxes' if pair else 'a box'} of consecutive x-planes: {who} module was built with x_planes")
        if getattr(self, "_shard_stripes", None) is not None:
            raise SafError(f"{call + ': ' if pair else ''}{who} volume holds only its reduce-scattered voxel stripes of a merged job; "
                           f"all_gather it (distributed.gather_shards, or merge_volumes(..., gather=True)) {before}")
        self._check_poisoned()

    def _retire_session(self):
        """The frames still queued belong to the box that is about to go: they are fused, and the queue's session, whose state is
        sized by that box, goes as in ``_apply``.  A deferred clear stays owed: no pass reads the row of a weight-0 voxel."""
        self._flush_pending(final=True)
        q = self.__dict__["_queue"]
        q.wait(self)
        q.close()

    def _new_box(self, origin, voxel_size, index_offset, nvox):
        """Buffers, axis tables and ``saf_volume`` of an empty box of that lattice, in this volume's widths and dtypes, on its device."""
        old = self._buffers
        dev = old["tsdf"].device
        n = nvox[0] * nvox[1] * nvox[2]
        new = {"tsdf": torch.zeros(n, dtype=torch.float32, device=dev),
               "rgb": torch.zeros((n, 3), dtype=torch.float32, device=dev),
               "weight": torch.zeros(n, dtype=torch.int32, device=dev),
               "tsdf_weight": torch.zeros(n, dtype=torch.int32, device=dev),
               # not cleared here: the rows of voxels that are still unwritten (weight 0) are zeroed when something first looks, by
               # the deferred clear of reset() -- the windowed path never reads them
               "clip_feat": torch.empty((n, int(self.n_clip_feats)), dtype=old["clip_feat"].dtype, device=dev)}
        labels = old.get("labels_one_hot")
        if labels is not None:
            new["labels_one_hot"] = torch.zeros((n, int(labels.shape[1])), dtype=torch.int32, device=dev)
        ax = [t.to(dev) for t in _axis_tables(origin, voxel_size, nvox, index_offset)]
        return new, ax, _volume_struct(new, ax, nvox, self.n_clip_feats, self.accum_mode, self.trunc)

    def _install_box(self, new, ax, nvox, index_offset, origin=None, voxel_size=None):
        """What ``_new_box`` made and a pass has filled becomes the module's volume: straight into ``_buffers`` (an assignment
        would pay the old volume's deferred clear first)."""
        b = self._buffers
        for name, t in new.items():
            b[name] = t
        b["axis_x"], b["axis_y"], b["axis_z"] = ax
        if "xyz_world" in b:
            b["xyz_world"] = _xyz_world(ax, nvox)
        self.nvox = torch.as_tensor(nvox, dtype=self.nvox.dtype)
        self.index_offset = index_offset
        if voxel_size is not None:
            self.voxel_size = voxel_size
        if origin is not None:
            self.origin = origin
        self.__dict__["_feat_stale"] = True  # (clip_feat was torch.empty)
        self._workspace = None  # (sized by the grid)
        self.__dict__["_shard16"] = None

    def _drop_labelling(self, keep_obj=False):
        """``voxel_obj_idx`` (unless ``keep_obj``) and ``objects_segmentation_color`` describe a labelling the volume no longer has."""
        for name in (() if keep_obj else ("voxel_obj_idx",)) + ("objects_segmentation_color",):
            if getattr(self, name, None) is not None:
                delattr(self, name)

    def move_grid(self, index_offset, nvox):
        """Move the volume to another box of ITS OWN lattice and keep what is fused: afterwards the module holds the ``nvox`` voxels
        that start at voxel index ``index_offset`` of the grid anchored at ``origin`` (offsets may be negative), and every voxel
        the old and the new box share holds, byte for byte, what it held before (saf_volume_carry, include/saf.h).
        Voxels the new box adds are empty, voxels it drops are lost.  Because the axis tables of two boxes of one lattice agree bit
        for bit on the indices they share, fusing further frames now gives, on the shared voxels, exactly the volume that would
        have held all the frames from the start.  ``origin``, ``voxel_size`` and ``trunc`` do not change; the module keeps its
        backbones, its queue and ``fuse_stats``.  Frames still queued behind ``integrate()`` are fused first.

        BOTH volumes are resident during the call: the new buffers are allocated before the old ones are let go.

        ``voxel_obj_idx``, if the caller has set one of the old grid's length, is carried along (-1 = no object in the voxels the new
        box adds); ``objects_segmentation_color`` is derived from it and is deleted: the caller recomputes it.  Returns a
        ``GridMove``; its counters are device tensors, nothing is read back here.  ``SafError``, with the volume unchanged, for a
        module built with ``x_planes``, one that holds only reduce-scattered stripes, a poisoned one, a non-positive ``nvox`` and a
        box of 2^31 voxels or more."""
        self._refuse_unfit("move_grid", "before moving it")
        new_off = tuple(int(v) for v in index_offset)
        new_nvox = tuple(int(v) for v in nvox)
        if len(new_off) != 3 or len(new_nvox) != 3 or min(new_nvox) <= 0:
            raise SafError(f"move_grid: nvox must be three positive sizes and index_offset three indices, got {new_nvox} at {new_off}")
        n_new = new_nvox[0] * new_nvox[1] * new_nvox[2]
        if n_new >= 1 << 31:
            raise SafError(f"move_grid: a box of {n_new} voxels (2^31 or more)")
        self._retire_session()
        old = dict(self._buffers)
        dev = old["tsdf"].device
        old_off, old_nvox = self.index_offset, tuple(int(v) for v in self.nvox)
        src = self._c_volume(for_fuse=True)  # (refuses a volume that is not on the device: no CPU fallback)
        obj = getattr(self, "voxel_obj_idx", None)
        if obj is not None and (not torch.is_tensor(obj) or obj.numel() != old["tsdf"].numel()):
            obj = None  # (not of this grid: left alone)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            new, ax, dst = self._new_box(self.origin, self.voxel_size, new_off, new_nvox)
            aux_src = aux_dst = None
            if obj is not None:
                aux_src = obj.to(device=dev, dtype=torch.int32).contiguous().reshape(-1)
                aux_dst = torch.full((n_new,), -1, dtype=torch.int32, device=dev)  # saf_label_components' "no object"
            counts = torch.zeros(2, dtype=torch.int64, device=dev)
            before = torch.stack(((old["weight"] > 0).sum(), (old["tsdf_weight"] > 0).sum()))
            off = tuple(new_off[a] - old_off[a] for a in range(3))
            check(lib().saf_volume_carry(C.byref(src), C.byref(dst), off[0], off[1], off[2], _abi.ptr(aux_src), _abi.ptr(aux_dst),
                                         _abi.ptr(counts), stream.cuda_stream), "saf_volume_carry")
            for t in list(old.values()) + ([aux_src] if aux_src is not None else []):
                t.record_stream(stream)  # (the old buffers are let go below; the pass reads them on this stream)
        self._install_box(new, ax, new_nvox, new_off)
        if obj is not None:
            self.voxel_obj_idx = aux_dst.view(*new_nvox) if obj.dim() == 3 else aux_dst
        self._drop_labelling(keep_obj=True)
        ext, in_old, in_new = _box_overlap(old_off, old_nvox, new_off, new_nvox)
        return GridMove(old_index_offset=old_off, old_nvox=old_nvox, index_offset=new_off, nvox=new_nvox, overlap_nvox=ext,
                        overlap_in_old=in_old, overlap_in_new=in_new, rows_carried=counts[0], rows_dropped=before[0] - counts[0],
                        tsdf_carried=counts[1], tsdf_dropped=before[1] - counts[1])

    def _absorb_refusals(self, other):
        """``absorb``'s refusals, decided before either volume is touched."""
        if other is self:
            raise SafError("absorb: a volume cannot absorb itself")
        if not isinstance(other, _GridOpsMixin):
            raise SafError(f"absorb: the other volume must be a fusion module, got {type(other).__name__}")
        for who, m in (("this", self), ("the other", other)):
            m._refuse_unfit("absorb", "first", who=who, pair=True)
        a, b = self._buffers, other._buffers
        if a["tsdf"].device != b["tsdf"].device:
            raise SafError(f"absorb: the volumes are on different devices ({a['tsdf'].device} and {b['tsdf'].device})")
        o_a = torch.as_tensor(self.origin).detach().cpu().to(torch.float32).reshape(-1)
        o_b = torch.as_tensor(other.origin).detach().cpu().to(torch.float32).reshape(-1)
        # (TSDF values are in units of trunc: blending two truncation distances would be wrong)
        if o_a.shape != o_b.shape or not torch.equal(o_a, o_b) or float(self.voxel_size) != float(other.voxel_size) or \
                float(self.trunc) != float(other.trunc):
            raise SafError("absorb: the volumes are not on the same lattice (origin, voxel_size and trunc must be equal): "
                           f"{o_a.tolist()} / {float(self.voxel_size)} / {float(self.trunc)} and "
                           f"{o_b.tolist()} / {float(other.voxel_size)} / {float(other.trunc)}")
        classes = lambda bufs: 0 if bufs.get("labels_one_hot") is None else int(bufs["labels_one_hot"].shape[1])
        if int(self.n_clip_feats) != int(other.n_clip_feats) or a["clip_feat"].dtype != b["clip_feat"].dtype or \
                classes(a) != classes(b) or bool(self._rgb_bilinear) != bool(other._rgb_bilinear):
            raise SafError("absorb: the volumes differ in feature width, feature dtype, classes or rgb sampling "
                           f"({int(self.n_clip_feats)} / {a['clip_feat'].dtype} / {classes(a)} / {bool(self._rgb_bilinear)} and "
                           f"{int(other.n_clip_feats)} / {b['clip_feat'].dtype} / {classes(b)} / {bool(other._rgb_bilinear)})")
        if self.accum_mode != _abi.SAF_RUNNING_MEAN or other.accum_mode != _abi.SAF_RUNNING_MEAN:
            raise SafError("absorb: running means only: a SAF_SUM volume belongs to the multi-rank job, whose merge adds its sums")

    def absorb(self, other, grow=True, multiple=4):
        """Take in what ``other`` -- a second module fused separately on the SAME lattice (equal ``origin``, ``voxel_size`` and
        ``trunc``; boxes that differ by whole voxels) -- has fused: per voxel and side, a count of 0 in ``other`` changes nothing, a
        count of 0 here takes ``other``'s values, and two positive counts blend by weights, the running mean of all the frames
        within fp32 rounding (saf_volume_absorb, include/saf.h).  ``other`` is only read and stays as it is.

        ``grow``: if ``other``'s box is not inside this one's, the volume is first moved (``move_grid``) to the box around both,
        ``nvox`` rounded up at the high end to a multiple of ``multiple`` as ``lattice_box`` does; with ``grow=False`` only the
        overlap is absorbed.  Frames still queued behind either module's ``integrate()`` are fused first; a deferred clear of
        either stays owed.  ``voxel_obj_idx`` and ``objects_segmentation_color`` describe a labelling the volume no longer has
        and are deleted.  Returns a ``GridAbsorb``; nothing is read back here.  ``SafError``, with both volumes unchanged, for
        ``other is self``, a module built with ``x_planes``, holding only reduce-scattered stripes or poisoned, another device,
        another lattice, a different feature width, feature dtype, class count or rgb sampling, and a ``SAF_SUM`` volume."""
        self._absorb_refusals(other)
        require_cuda(self._buffers["clip_feat"], "the fusion volume")
        # the queued frames of both; the other's session only finishes.  A deferred clear of either stays owed: the pass reads no
        # row of a weight-0 voxel, and writes every row whose voxel gains a weight
        self._retire_session()
        other._flush_pending(final=True)
        other.__dict__["_queue"].wait(other)
        o_off, o_n = other.index_offset, tuple(int(v) for v in other.nvox)
        s_off, s_n = self.index_offset, tuple(int(v) for v in self.nvox)
        move = None
        if grow and not all(s_off[a] <= o_off[a] and o_off[a] + o_n[a] <= s_off[a] + s_n[a] for a in range(3)):
            m = max(int(multiple), 1)
            lo = tuple(min(s_off[a], o_off[a]) for a in range(3))
            hi = tuple(max(s_off[a] + s_n[a], o_off[a] + o_n[a]) for a in range(3))
            move = self.move_grid(lo, tuple((hi[a] - lo[a] + m - 1) // m * m for a in range(3)))
            s_off, s_n = self.index_offset, tuple(int(v) for v in self.nvox)
        # (_buffers, never attribute access: that would pay a deferred clear)
        dev = self._buffers["tsdf"].device
        ob = other._buffers
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            counts = torch.zeros(4, dtype=torch.int64, device=dev)
            before = torch.stack(((ob["weight"] > 0).sum(), (ob["tsdf_weight"] > 0).sum()))
            off = tuple(s_off[a] - o_off[a] for a in range(3))
            check(lib().saf_volume_absorb(C.byref(other._c_volume(for_fuse=True)), C.byref(self._c_volume(for_fuse=True)), off[0],
                                          off[1], off[2], _abi.ptr(counts), stream.cuda_stream), "saf_volume_absorb")
        self.__dict__["_shard16"] = None
        self._drop_labelling()
        ext, in_self, in_other = _box_overlap(s_off, s_n, o_off, o_n)
        return GridAbsorb(index_offset=s_off, nvox=s_n, other_index_offset=o_off, other_nvox=o_n, overlap_nvox=ext,
                          overlap_in_self=in_self, overlap_in_other=in_other, move=move, rows_blended=counts[0], rows_copied=counts[1], tsdf_blended=counts[2], tsdf_copied=counts[3],
                          rows_outside=before[0] - counts[0] - counts[1], tsdf_outside=before[1] - counts[2] - counts[3])

    def coarsen(self, factor=2):
        """Coarsen the volume IN PLACE by a whole ``factor`` (2, 3 or 4) on block boundaries of its lattice and keep fusing at the
        coarse size: a coarse voxel is the weighted mean of the ``factor``^3 fine voxels it covers -- global coarse index I covers
        the fine global indices ``factor * I .. factor * I + factor - 1`` (saf_volume_coarsen, include/saf.h).
        Afterwards ``voxel_size`` is ``factor`` times what it was, ``origin`` is the centre of the block of global coarse index 0
        (``coarse_lattice``: it depends on the old origin, voxel size and factor only, so two boxes of one lattice coarsen onto
        one coarse lattice and can be ``absorb``ed), ``index_offset`` and ``nvox`` are the blocks the old box touches; ``trunc``
        does not change.  The stored counts are the MAXIMA over a block's children, not the sums: a later frame's sample stays
        worth one frame.  The module keeps its backbones, its queue and ``fuse_stats``; frames still queued behind ``integrate()``
        are fused first; a deferred clear stays owed.

        Frames fused before the call can no longer be taken out with ``deintegrate``: their samples are spread over other voxels
        at other weights.  The module keeps no ledger of what it holds, so that is the caller's business, as after ``absorb`` on
        16-bit volumes.

        BOTH volumes are resident during the call.  ``voxel_obj_idx`` and ``objects_segmentation_color`` describe a labelling of
        the fine grid and are deleted.  Returns a ``GridCoarsen``; its counters are device tensors, nothing is read back here.
        ``SafError``, with the volume unchanged, for a module built with ``x_planes``, one that holds only reduce-scattered
        stripes, a poisoned one, a ``SAF_SUM`` volume, and a factor that is not the int 2, 3 or 4."""
        self._refuse_unfit("coarsen", "before coarsening it")
        if self.accum_mode != _abi.SAF_RUNNING_MEAN:
            raise SafError("coarsen: running means only: a SAF_SUM volume belongs to the multi-rank job, whose merge adds its sums")
        if isinstance(factor, bool) or not isinstance(factor, int) or factor not in (2, 3, 4):
            raise SafError(f"coarsen: the factor must be the int 2, 3 or 4, got {factor!r}")
        self._retire_session()
        old = dict(self._buffers)
        dev = old["tsdf"].device
        old_off, old_nvox = self.index_offset, tuple(int(v) for v in self.nvox)
        old_origin, old_vs = self.origin, self.voxel_size
        new_origin, new_vs, new_off, new_nvox = coarse_lattice(old_origin, old_vs, old_off, old_nvox, factor)
        src = self._c_volume(for_fuse=True)  # (refuses a volume that is not on the device: no CPU fallback)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            new, ax, dst = self._new_box(new_origin, new_vs, new_off, new_nvox)
            counts = torch.zeros(4, dtype=torch.int64, device=dev)
            check(lib().saf_volume_coarsen(C.byref(src), C.byref(dst), factor, old_off[0], old_off[1], old_off[2], _abi.ptr(counts),
                                           stream.cuda_stream), "saf_volume_coarsen")
            for t in old.values():
                t.record_stream(stream)  # (the old buffers are let go below; the pass reads them on this stream)
        self._install_box(new, ax, new_nvox, new_off, origin=new_origin, voxel_size=new_vs)
        self._drop_labelling()
        return GridCoarsen(factor=factor, old_origin=old_origin, old_voxel_size=old_vs, old_index_offset=old_off, old_nvox=old_nvox,
                           origin=new_origin, voxel_size=new_vs, index_offset=new_off, nvox=new_nvox,
                           rows_blended=counts[0], rows_copied=counts[1], tsdf_blended=counts[2], tsdf_copied=counts[3])

    def resample(self, origin=None, voxel_size=None, index_offset=None, nvox=None, transform=None, lattice_of=None, min_cover=0.5,
                 multiple=4):
        """Resample the volume IN PLACE onto any other lattice -- another ``origin``, any ``voxel_size`` (finer, or coarser by any
        factor), and a rigid ``transform`` (4 x 4 ``new_from_old``: a world point x of the frame the volume was fused in is
        ``transform @ x`` in the new one; default the identity) -- and keep fusing there: every new voxel looks up the eight old
        voxels around its own centre and blends the observed ones by their trilinear weights, renormalised; a voxel whose
        observed corners cover less than ``min_cover`` of the trilinear weight stays empty, so that no surface grows a fringe
        (saf_volume_resample, include/saf.h).  ``lattice_of``: another fusion module, or a ``SceneResult``, whose
        ``origin`` and ``voxel_size`` are taken (then neither may be given) -- afterwards ``lattice_of.absorb(self)`` is accepted,
        the two-headset flow with ``transform`` from ``refine_pose``.  ``origin`` / ``voxel_size`` default to the module's own.
        ``index_offset`` and ``nvox``, the new box on the new lattice, are given together or come from ``resample_box`` (the box
        around the transformed old box, ``nvox`` rounded up to a multiple of ``multiple``).  ``trunc`` does not change: TSDF
        values are in units of it, which is why a transform that scales is refused.

        The stored counts are the MAXIMA over the contributing corners; a label histogram is copied from the heaviest corner.
        Trilinear interpolation low-passes the features by up to one old voxel.  Frames fused before the call can no longer be
        taken out with ``deintegrate``, as after ``coarsen``; poses handed to ``integrate()`` afterwards are the caller's, in the
        NEW frame.  The module keeps its backbones, its queue and ``fuse_stats``; frames still queued behind ``integrate()`` are
        fused first; a deferred clear stays owed.

        BOTH volumes are resident during the call.  ``voxel_obj_idx`` and ``objects_segmentation_color`` describe a labelling of
        the old grid and are deleted.  Returns a ``GridResample``; its counters are device tensors, nothing is read back here.
        ``SafError``, with the volume unchanged, for a module built with ``x_planes``, one that holds only reduce-scattered
        stripes, a poisoned one, a ``SAF_SUM`` volume, a transform that is not 4 x 4, finite and rigid, a non-positive
        ``voxel_size``, a box that is not three positive sizes at three indices or holds 2^31 voxels or more, and a ``min_cover``
        outside (0, 1]."""
        self._refuse_unfit("resample", "before resampling it")
        if self.accum_mode != _abi.SAF_RUNNING_MEAN:
            raise SafError("resample: running means only: a SAF_SUM volume belongs to the multi-rank job, whose merge adds its sums")
        if lattice_of is not None:
            if origin is not None or voxel_size is not None:
                raise SafError("resample: lattice_of gives the origin and the voxel size; pass neither of them with it")
            base = getattr(lattice_of, "fusion", lattice_of)
            if not isinstance(base, _GridOpsMixin):
                raise SafError(f"resample: lattice_of must be a fusion module or a SceneResult, got {type(lattice_of).__name__}")
            origin, voxel_size = base.origin, base.voxel_size
        new_origin = self.origin if origin is None else origin
        new_vs = self.voxel_size if voxel_size is None else voxel_size
        t64 = _rigid_transform(transform)
        o64 = _origin64(new_origin)
        try:
            vs_ok = not isinstance(new_vs, bool) and np.isfinite(float(new_vs)) and float(new_vs) > 0
        except (TypeError, ValueError):
            vs_ok = False
        if not vs_ok:
            raise SafError(f"resample: the voxel size must be a positive number, got {new_vs!r}")
        try:
            cover_ok = not isinstance(min_cover, bool) and 0.0 < float(min_cover) <= 1.0
        except (TypeError, ValueError):
            cover_ok = False
        if not cover_ok:
            raise SafError(f"resample: min_cover must lie in (0, 1], got {min_cover!r}")
        if (index_offset is None) != (nvox is None):
            raise SafError("resample: index_offset and nvox are given together, or neither")
        if nvox is None:
            new_off, new_nvox = resample_box(self, o64, new_vs, t64, multiple=multiple)
        else:
            try:
                new_off, new_nvox = tuple(int(v) for v in index_offset), tuple(int(v) for v in nvox)
            except (TypeError, ValueError):
                new_off, new_nvox = (), ()
            if len(new_off) != 3 or len(new_nvox) != 3 or min(new_nvox) <= 0:
                raise SafError(f"resample: nvox must be three positive sizes and index_offset three indices, got {nvox!r} at {index_offset!r}")
        n_new = new_nvox[0] * new_nvox[1] * new_nvox[2]
        if n_new >= 1 << 31:
            raise SafError(f"resample: a box of {n_new} voxels (2^31 or more)")
        self._retire_session()
        old = dict(self._buffers)
        dev = old["tsdf"].device
        old_off, old_nvox = self.index_offset, tuple(int(v) for v in self.nvox)
        old_origin, old_vs = self.origin, self.voxel_size
        m12 = resample_matrix(old_origin, old_vs, old_off, o64, new_vs, new_off, t64)
        src = self._c_volume(for_fuse=True)  # (refuses a volume that is not on the device: no CPU fallback)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            new, ax, dst = self._new_box(new_origin, new_vs, new_off, new_nvox)
            counts = torch.zeros(4, dtype=torch.int64, device=dev)
            # (the matrix is host memory, read during the call)
            check(lib().saf_volume_resample(C.byref(src), C.byref(dst), _abi.ptr(m12), float(min_cover), _abi.ptr(counts),
                                            stream.cuda_stream), "saf_volume_resample")
            for t in old.values():
                t.record_stream(stream)  # (the old buffers are let go below; the pass reads them on this stream)
        self._install_box(new, ax, new_nvox, new_off, origin=new_origin, voxel_size=new_vs)
        self._drop_labelling()
        return GridResample(old_origin=old_origin, old_voxel_size=old_vs, old_index_offset=old_off, old_nvox=old_nvox,
                            origin=new_origin, voxel_size=new_vs, index_offset=new_off, nvox=new_nvox, transform=t64, matrix=m12,
                            min_cover=float(min_cover), rows_blended=counts[0], rows_copied=counts[1], tsdf_blended=counts[2],
                            tsdf_copied=counts[3])


def lattice_box(fusion, xyz, trunc_m=None, union=True, multiple=4):
    """The box of ``fusion``'s own lattice for the sparse cloud ``xyz`` -- what ``move_grid`` takes: (index_offset, nvox), tuples
    of ints.  The bounds are ``scene_bounds``'s (1st / 99th percentile -/+ ``trunc_m``, default the module's ``trunc``), snapped
    OUTWARD to the lattice in float64 -- the lattice index of a coordinate c is (c - origin) / voxel_size; floor for the low corner,
    ceil for the high one, so the first voxel centre is at or below the low bound and the last at or above the high one --, united
    with the module's current box (``union``), and ``nvox`` rounded up per axis, at the high end, to a multiple of ``multiple``
    (the windowed path's bricks are 4 x 4 x 16 voxels; 1: as snapped).  Offsets may be negative.  Host only."""
    pts = xyz.cpu().numpy() if isinstance(xyz, torch.Tensor) else np.asarray(xyz)
    trunc_m = float(fusion.trunc if trunc_m is None else trunc_m)
    origin = torch.as_tensor(fusion.origin).detach().cpu().numpy().astype(np.float64)
    vs = float(fusion.voxel_size)
    lo = np.floor((np.percentile(pts, 1, axis=0).astype(np.float64) - trunc_m - origin) / vs).astype(np.int64)
    hi = np.ceil((np.percentile(pts, 99, axis=0).astype(np.float64) + trunc_m - origin) / vs).astype(np.int64)
    if union:
        off, nvox = np.asarray(fusion.index_offset, dtype=np.int64), np.asarray([int(v) for v in fusion.nvox], dtype=np.int64)
        lo, hi = np.minimum(lo, off), np.maximum(hi, off + nvox - 1)
    n = hi - lo + 1
    m = max(int(multiple), 1)
    n = (n + m - 1) // m * m
    return tuple(int(v) for v in lo), tuple(int(v) for v in n)


def coarse_lattice(origin, voxel_size, index_offset, nvox, factor):
    """What ``coarsen`` makes of a box of a lattice: (origin', voxel_size', index_offset', nvox').  Global coarse voxel I covers the
    fine global indices ``factor * I .. factor * I + factor - 1`` (floor division: blocks are aligned to the lattice, not to the
    box), so ``voxel_size' = factor * voxel_size``, ``origin' = origin + 0.5 * (factor - 1) * voxel_size`` -- the centre of the block
    of global coarse index 0, computed in float64 and returned in the container and dtype ``origin`` came in --, ``index_offset' =
    floor(off / factor)`` and ``nvox' = ceil((off + n) / factor) - floor(off / factor)`` per axis.  ``origin'`` does not depend on
    the box: two boxes of one fine lattice give two boxes of one coarse lattice.  Host only."""
    f = int(factor)
    off = tuple(int(v) for v in index_offset)
    n = tuple(int(v) for v in nvox)
    new_off = tuple(o // f for o in off)  # (Python's // is the floor division)
    new_n = tuple(-((-(o + k)) // f) - o // f for o, k in zip(off, n))
    o64 = torch.as_tensor(origin).detach().cpu().to(torch.float64) + 0.5 * (f - 1) * float(voxel_size)
    if torch.is_tensor(origin):
        new_origin = o64.to(dtype=origin.dtype, device=origin.device)
    elif isinstance(origin, np.ndarray):
        new_origin = o64.numpy().astype(origin.dtype)
    else:
        new_origin = type(origin)(o64.tolist())
    return new_origin, f * voxel_size, new_off, new_n


def _origin64(origin):
    """A lattice's origin as three float64."""
    o = torch.as_tensor(origin).detach().cpu().to(torch.float64).reshape(-1).numpy()
    if o.shape != (3,) or not np.isfinite(o).all():
        raise SafError(f"resample: the origin must be three finite coordinates, got {origin!r}")
    return o


def _rigid_transform(transform):
    """``transform`` (None: the identity) as a 4 x 4 float64 array; ``SafError`` unless it is 4 x 4, finite and rigid: a last row of
    0 0 0 1, max |R^T R - I| <= 1e-6 and det R > 0, decided in float64 (a scale would change what a TSDF value means: TSDF values
    are in units of ``trunc``, which stays)."""
    if transform is None:
        return np.eye(4)
    try:
        t = transform.detach().cpu().to(torch.float64).numpy() if torch.is_tensor(transform) else np.asarray(transform, dtype=np.float64)
    except (TypeError, ValueError):
        raise SafError(f"resample: the transform must be a 4 x 4 matrix, got {type(transform).__name__}") from None
    if t.shape != (4, 4) or not np.isfinite(t).all():
        raise SafError(f"resample: the transform must be a finite 4 x 4 matrix (new_from_old), got shape {tuple(t.shape)}")
    r = t[:3, :3]
    if not np.array_equal(t[3], np.array([0.0, 0.0, 0.0, 1.0])) or float(np.abs(r.T @ r - np.eye(3)).max()) > 1e-6 or \
            float(np.linalg.det(r)) <= 0:
        raise SafError("resample: the transform is not rigid (last row 0 0 0 1, max |R^T R - I| <= 1e-6, det R > 0): scale, shear and "
                       "reflections are refused")
    return np.array(t, dtype=np.float64)


def resample_matrix(src_origin, src_vs, src_off, dst_origin, dst_vs, dst_off, transform=None):
    """The [3, 4] float32 matrix ``saf_volume_resample`` takes: a destination voxel's LOCAL index i (its own box, from 0) to the
    continuous local index p of the source box.  From the centre ``world_new = (i + dst_off) * dst_vs + dst_origin``:
    ``world_old = inv(transform) @ world_new`` (``transform``: 4 x 4 rigid ``new_from_old``; None: the identity) and
    ``p = (world_old - src_origin) / src_vs - src_off`` -- composed in float64 and rounded ONCE to float32.  Host only."""
    t = np.eye(4) if transform is None else (transform.detach().cpu().to(torch.float64).numpy() if torch.is_tensor(transform)
                                             else np.asarray(transform, dtype=np.float64))
    so, do = _origin64(src_origin), _origin64(dst_origin)
    s_vs, d_vs = float(src_vs), float(dst_vs)
    s_off, d_off = np.asarray([int(v) for v in src_off], dtype=np.float64), np.asarray([int(v) for v in dst_off], dtype=np.float64)
    inv = np.linalg.inv(t)
    m = np.empty((3, 4), dtype=np.float64)
    m[:, :3] = inv[:3, :3] * (d_vs / s_vs)
    # (the whole-voxel part apart from the origins' part: with the identity on one lattice the column is dst_off - src_off exactly,
    #  every p is a whole number and the pass is a copy)
    m[:, 3] = (m[:, :3] @ d_off + (inv[:3, :3] @ do + inv[:3, 3] - so) / s_vs) - s_off
    return np.ascontiguousarray(m.astype(np.float32))


def resample_box(fusion, origin, voxel_size, transform=None, multiple=4):
    """The box of the lattice (``origin``, ``voxel_size``) around ``fusion``'s current box under ``transform`` (4 x 4 rigid
    ``new_from_old``; None: the identity) -- what ``resample`` takes when no box is given: (index_offset, nvox), tuples of ints.
    The eight corners of the current box (the centres of its corner voxels: beyond them there is nothing to interpolate) are
    transformed and snapped OUTWARD to the lattice in float64 as ``lattice_box`` snaps -- the lattice index of a coordinate c is
    (c - origin) / voxel_size; floor for the low corner, ceil for the high one --, and ``nvox`` is rounded up per axis, at the
    high end, to a multiple of ``multiple`` (1: as snapped).  Offsets may be negative.  Host only."""
    t = _rigid_transform(transform)
    o_new, vs_new = _origin64(origin), float(voxel_size)
    o_old, vs_old = _origin64(fusion.origin), float(fusion.voxel_size)
    off = np.asarray(fusion.index_offset, dtype=np.float64)
    n = np.asarray([int(v) for v in fusion.nvox], dtype=np.float64)
    corners = np.array([[off[a] + (n[a] - 1) * ((k >> (2 - a)) & 1) for a in range(3)] for k in range(8)])
    # (the whole-voxel part apart from the origins' part, as in resample_matrix: on the own lattice the box is the own box exactly)
    idx = corners @ (t[:3, :3] * (vs_old / vs_new)).T + (t[:3, :3] @ o_old + t[:3, 3] - o_new) / vs_new
    lo = np.floor(idx.min(axis=0)).astype(np.int64)
    hi = np.ceil(idx.max(axis=0)).astype(np.int64)
    m = max(int(multiple), 1)
    size = (hi - lo + 1 + m - 1) // m * m
    return tuple(int(v) for v in lo), tuple(int(v) for v in size)
