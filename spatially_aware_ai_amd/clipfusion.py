"""Host-side mirror of the reference's ``clipfusion.py`` hot-path API on MI355X.

Same names, arguments and error behaviour as the reference classes so that its callers
(`run_clipfusion`, `InSituManager`, `query_mesh.py`, the eval scripts) can switch imports:

  * ``ClipFusion``      -- reference clipfusion.py:575-763 (volume + ``integrate``)
  * ``Clip``            -- reference clipfusion.py:766-1039 (tiled image features, text query head)
  * ``backproject_pcd`` -- reference clipfusion.py:510-572
  * ``get_pix_vecs``    -- reference clipfusion.py:497-507
  * ``scene_bounds``    -- the bounds arithmetic of clipfusion.py:1098-1106
  * ``lattice_box`` / ``move_grid`` -- not in the reference: a volume moved by whole voxels on its own lattice
  * ``absorb`` -- not in the reference: a second volume of the same lattice blended in by weights
  * ``coarsen`` / ``coarse_lattice`` -- not in the reference: a volume coarsened by a whole factor on its lattice;
  * ``resample`` / ``resample_matrix`` / ``resample_box`` -- not in the reference: a volume resampled onto any other lattice under a
    rigid transform; these four live in ``_grid_ops.py``

PyTorch is plumbing here (device memory, streams, the backbone GEMMs); the fusion loop and the
query scan are the hand-written HIP kernels behind ``include/saf.h``.  There is no CPU
fallback: tensors that are not on the HIP device raise.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from . import _abi
from ._carve import CarveResult, FreeSpaceEvidence, _CarveMixin, erode_depth  # noqa: F401
from ._frame_queue import FrameQueue, StagingRing
from ._grid_ops import (_DT, GridAbsorb, GridCoarsen, GridMove, GridResample, _axis_tables, _GridOpsMixin,  # noqa: F401
                        _volume_struct, _xyz_world, coarse_lattice, lattice_box, resample_box, resample_matrix)
from ._lib import SafError, check, current_stream_ptr, lib, require_cuda

_FRAME_WORDS = C.sizeof(_abi.SafFrame) // 8
assert C.sizeof(_abi.SafFrame) == 72 and _abi.SafFrame.depth.offset == 8 and _abi.SafFrame.npy.offset == 48 and \
    _abi.SafFrame.label_map.offset == 56 and _abi.SafFrame.rgb_bilinear.offset == 64, "struct saf_frame layout (include/saf.h)"

# --------------------------------------------------------------------------------------------
# volume plumbing shared by ClipFusion and ClipSeemFusion
# --------------------------------------------------------------------------------------------


# `fusion.borrow_inputs = True` (default: SAF_BORROW_INPUTS=1 in the environment, else False): the queue behind integrate() does
# not copy a call's depth / rgb / label images into its staging ring but reads them where they are when their window is fused --
# up to 512 frames later.  The caller promises not to WRITE those tensors until flush() (dropping them is fine: the queue holds
# them); the reference's loop (a fresh batch per DataLoader step, clip_seem_fusion.py:303-313) keeps that promise by construction.
_BORROW_DEFAULT = os.environ.get("SAF_BORROW_INPUTS", "0") == "1"
_VOLUME_BUFFERS = frozenset(("tsdf", "rgb", "clip_feat", "weight", "tsdf_weight", "labels_one_hot", "fuse_stats"))


class _FusionVolumeMixin(_GridOpsMixin, _CarveMixin):
    """Buffers, workspace and the C-ABI call shared by both fusion modules (``move_grid``, ``absorb``, ``coarsen`` and ``resample``:
    _grid_ops.py; ``observe_free_space`` and ``carve``: _carve.py)."""

    def _init_volume(self, origin, voxel_size, nvox, trunc, feat_dim, n_classes=0, keep_xyz_world=True,
                     feat_dtype=torch.float32, index_offset=(0, 0, 0), x_planes=None, device=None):
        """``device`` (not in the reference): create the buffers there instead of on the host.  The reference builds its module on
        the host and moves it (clipfusion.py:1119, clip_seem_fusion.py:291-302) -- gigabytes of zeros through pageable memory
        (0.7 s at 127 x 104 x 116 x 512); the axis tables are computed on the host either way."""
        zeros = lambda *a, **k: torch.zeros(*a, device=device, **k)
        nvox = torch.as_tensor(nvox)
        n = int(torch.prod(nvox.long()))
        self.origin = origin
        self.voxel_size = voxel_size
        self.nvox = nvox
        self.trunc = trunc
        self.n_clip_feats = feat_dim
        self.accum_mode = _abi.SAF_RUNNING_MEAN
        self.register_buffer("tsdf", zeros(n, dtype=torch.float32))
        self.register_buffer("rgb", zeros((n, 3), dtype=torch.float32))
        if feat_dtype not in _DT:
            raise ValueError("feat_dtype must be torch.float32 (the reference layout), torch.bfloat16 or torch.float16")
        self.register_buffer("clip_feat", zeros((n, feat_dim), dtype=feat_dtype))
        self.register_buffer("weight", zeros(n, dtype=torch.int32))
        self.register_buffer("tsdf_weight", zeros(n, dtype=torch.int32))
        if n_classes:
            self.register_buffer("labels_one_hot", zeros((n, n_classes), dtype=torch.int32))
        self.index_offset = tuple(int(v) for v in index_offset)
        self.x_planes = None if x_planes is None else torch.as_tensor(x_planes, dtype=torch.int64).detach().cpu().clone()
        ax = _axis_tables(origin, voxel_size, nvox, self.index_offset, self.x_planes)
        if device is not None:
            ax = [t.to(device) for t in ax]
        # not in the reference's state_dict: derived tables the sweep kernel reads instead of xyz_world
        self.register_buffer("axis_x", ax[0], persistent=False)
        self.register_buffer("axis_y", ax[1], persistent=False)
        self.register_buffer("axis_z", ax[2], persistent=False)
        self.register_buffer("fuse_stats", zeros(_abi.SAF_STATS_WORDS, dtype=torch.int64), persistent=False)
        if keep_xyz_world:
            self.register_buffer("xyz_world", _xyz_world(ax, nvox))
        self._workspace = None
        self._shard_stripes = None  # [(first, count)] while the volume holds only its reduce-scattered stripes of a merged job
        self.__dict__.setdefault("defer_frames", True)  # queue small integrate() calls into 128-frame windows
        self.__dict__["_feat_stale"] = False
        # the queue behind integrate() (_frame_queue.py).  Not a registered buffer, so reading it never enters __getattr__; until
        # this line has run there is none, and "no queue yet" reads as "idle" (__setattr__ is reached above)
        self.__dict__["_queue"] = FrameQueue()

    def __del__(self):
        q = self.__dict__.get("_queue")
        if q is not None:
            try:
                q.close()  # (destroys the session)
            except Exception:  # noqa: BLE001 -- interpreter shutdown
                pass

    # -- C structs -------------------------------------------------------------------------
    def _c_volume(self, for_fuse=False):
        """The saf_volume descriptor of the buffers.  ``for_fuse``: for the fuse kernels themselves -- neither the
        queued frames nor the deferred clear (reset) are resolved first."""
        if not for_fuse:
            self._sync_volume()
        b = self._buffers
        require_cuda(b["clip_feat"], "the fusion volume")
        for name in ("tsdf", "rgb", "clip_feat", "weight", "tsdf_weight"):
            if not b[name].is_contiguous():
                raise SafError(f"buffer {name} must be contiguous")
        return _volume_struct(b, (b["axis_x"], b["axis_y"], b["axis_z"]), self.nvox, self.n_clip_feats, self.accum_mode, self.trunc)

    def _get_workspace(self, npy, npx, hw=None):
        """``hw`` = (height, width) of the frames: a volume of a million voxels or more also gets room for the windowed path's
        tiled depth copies (0.63 GB at 640 x 480; half the classification's cache lines); the library falls back to
        the frames' own images when the room is not there -- results are identical either way."""
        tsdf = self._buffers["tsdf"]
        n = tsdf.numel()
        # for THIS volume (width, dtype, SAF_WIN_FORM): the brick form's 6.5 GB of segment pools only where it would run
        # (SAF_TILED_MIN_VOXELS, read per call: the tests ask for the tiled copies on small volumes)
        if hw is not None and n >= int(os.environ.get("SAF_TILED_MIN_VOXELS", 1 << 20)):
            need = lib().saf_fuse_workspace_bytes_for_frames(C.byref(self._c_volume(for_fuse=True)), int(npy), int(npx),
                                                             int(hw[0]), int(hw[1]))
        else:
            need = lib().saf_fuse_workspace_bytes_for(C.byref(self._c_volume(for_fuse=True)), int(npy), int(npx))
        ws = self._workspace
        if ws is None or ws.numel() < need or ws.device != tsdf.device:
            ws = torch.empty(need, dtype=torch.uint8, device=tsdf.device)
            self._workspace = ws
        return ws

    @staticmethod
    def _f32c(t, name):
        require_cuda(t, name)
        if t.dtype != torch.float32:
            t = t.float()
        return t.contiguous()

    def _make_frames(self, depth_imgs, rgb_imgs, poses, K, clip_feat_img, label_maps, rgb_bilinear, borrowed=None):
        """C descriptors for a batch; returns (ctypes array, keepalive list, npy, npx).  ``borrowed`` ([B, 3] int64, or None):
        per frame the addresses of a caller's depth / rgb / label images that stand in for the batch's (0: none)."""
        depth_imgs = self._f32c(depth_imgs, "depth_imgs")
        rgb_imgs = self._f32c(rgb_imgs, "rgb_imgs")
        poses = self._f32c(poses, "poses")
        K = self._f32c(K, "K")
        feat = self._f32c(clip_feat_img, "clip feature map")
        bsz, h, w = depth_imgs.shape
        if rgb_imgs.shape != (bsz, h, w, 3):
            raise ValueError(f"rgb_imgs must be [B,H,W,3], got {tuple(rgb_imgs.shape)}")
        if poses.shape != (bsz, 4, 4) or K.shape != (bsz, 3, 3):
            raise ValueError("poses must be [B,4,4] and K [B,3,3]")
        if feat.dim() != 4 or feat.shape[0] != bsz or feat.shape[1] < self.n_clip_feats:
            raise ValueError(f"feature map must be [B,D>={self.n_clip_feats},npy,npx], got {tuple(feat.shape)}")
        labs = lab_ptrs = None
        if torch.is_tensor(label_maps):  # one [B,H,W] tensor (the staging ring)
            labs = self._f32c(label_maps, "label maps")
            if labs.shape != (bsz, h, w):
                raise ValueError("label maps must be [B,H,W]")
            lab_ptrs = labs.data_ptr() + np.arange(bsz, dtype=np.int64) * (4 * h * w)
            labs = [labs]
        elif label_maps is not None:
            labs = [self._f32c(m, "label map") for m in label_maps]
            for m in labs:
                if m.shape != (h, w):
                    raise ValueError("label map must be [H,W]")
            lab_ptrs = np.fromiter((m.data_ptr() for m in labs), dtype=np.int64, count=bsz)
        npy, npx = int(feat.shape[2]), int(feat.shape[3])
        # the descriptors as int64 words (struct saf_frame, include/saf.h: 72 bytes), filled column by column: a Python
        # object per frame and field would be thousands of short-lived objects per flush -- garbage-collector pauses
        # in the middle of the one-frame-per-call loop
        arr = np.zeros((bsz, _FRAME_WORDS), dtype=np.int64)
        idx = np.arange(bsz, dtype=np.int64)
        arr[:, 0] = h | (w << 32)
        arr[:, 1] = depth_imgs.data_ptr() + idx * (4 * h * w)
        arr[:, 2] = rgb_imgs.data_ptr() + idx * (12 * h * w)
        arr[:, 3] = poses.data_ptr() + idx * 64
        arr[:, 4] = K.data_ptr() + idx * 36
        arr[:, 5] = feat.data_ptr() + idx * (4 * int(feat.shape[1]) * npy * npx)
        arr[:, 6] = npy | (npx << 32)
        if lab_ptrs is not None:
            arr[:, 7] = lab_ptrs
        arr[:, 8] = int(bool(rgb_bilinear))
        if borrowed is not None:
            for col, k in ((1, 0), (2, 1), (7, 2)):
                arr[:, col] = np.where(borrowed[:, k] != 0, borrowed[:, k], arr[:, col])
        return (_abi.SafFrame * bsz).from_buffer(arr), (depth_imgs, rgb_imgs, poses, K, feat, labs), npy, npx

    # -- the deferred window queue ---------------------------------------------------------------
    # (what it is and why: _frame_queue.py, which owns its state; here are the decisions -- queue or fuse now, what a flush hands
    #  over, session or one call -- and the knobs, readable and overridable per instance)
    _DEFER_MAX_BATCH = 15  # calls of 16+ frames take the windowed path by themselves
    # up to four windows per flush (from the second one on, a window is classified beside its predecessor's rows); a full
    # window is flushed earlier when the device has finished the previous flush and would otherwise idle
    _QUEUE_FRAMES = 4 * _abi.SAF_WINDOW_FRAMES
    _PUSH_FRAMES = 32  # frames of one classification launch (one mask plane of a window): the unit the session takes

    def _defer_ok(self, bsz, npy, npx):
        if not self.__dict__.get("defer_frames", True) or bsz > self._DEFER_MAX_BATCH:
            return False
        d = int(self.n_clip_feats)
        rows16 = self._buffers["clip_feat"].dtype != torch.float32  # bf16 and fp16 rows: 8 channels per 16-byte unit
        # the shapes saf_fuse_frames takes on the windowed path (include/saf.h); others gain nothing from a queue
        return d <= 1024 and d % (512 if rows16 else 256) == 0 and npy + 3 <= 255 and npx + 3 <= 255

    def _fuse(self, depth_imgs, rgb_imgs, poses, K, clip_feat_img, label_maps=None, rgb_bilinear=False, lazy_feat=None):
        """``lazy_feat`` = (fn, (C, npy, npx)) instead of ``clip_feat_img``: the feature maps of these frames are
        ``fn(rgb[n,H,W,3]) -> [n,C,npy,npx]`` and may be computed later -- when the queue is flushed, for all queued frames in
        one backbone batch (the reference feeds its ViT 35 tiles per call; a flush feeds it 128 x 35)."""
        bsz = int(depth_imgs.shape[0])
        f32 = torch.float32
        if getattr(self, "_shard_stripes", None) is not None:
            # refused HERE, not when the queue is flushed: a queued frame would make every later read of the volume raise
            raise SafError(
                "this volume holds only its reduce-scattered voxel stripes of a merged job; all_gather it "
                "(distributed.gather_shards, or merge_volumes(..., gather=True)) before fusing more frames"
            )
        if self.accum_mode == _abi.SAF_SUM and self._buffers["clip_feat"].dtype == torch.float16:
            # (saf_fuse_frames refuses it too; here, so that no such frame is ever queued)
            raise SafError("SAF_SUM into an fp16 volume is not supported: sums over many frames leave fp16's range (65504) and "
                           "saf_merge_finalize takes fp32 sums only -- accumulate in torch.float32")
        if clip_feat_img is None:
            fn, fshape = lazy_feat
            lazy_ok = self._defer_ok(bsz, fshape[1], fshape[2]) and all(
                t.is_cuda and t.dtype == f32 and t.is_contiguous() for t in (depth_imgs, rgb_imgs, poses, K)) and (
                label_maps is None or all(m.is_cuda and m.dtype == f32 and m.is_contiguous() for m in label_maps))
            if not lazy_ok:
                return self._fuse(depth_imgs, rgb_imgs, poses, K, fn(rgb_imgs), label_maps, rgb_bilinear)
            # the backbone runs at flush time: under the autocast state of THIS call
            lazy = (fn, bool(torch.is_autocast_enabled("cuda")), torch.get_autocast_dtype("cuda"))
        else:
            lazy = None
            if clip_feat_img.dim() != 4 or not self._defer_ok(bsz, int(clip_feat_img.shape[2]), int(clip_feat_img.shape[3])):
                self._flush_pending(final=True)  # (frames are fused in call order)
                return self._fuse_now(depth_imgs, rgb_imgs, poses, K, clip_feat_img, label_maps, rgb_bilinear)
            fshape = tuple(int(v) for v in clip_feat_img.shape[1:])
        h, w = int(depth_imgs.shape[1]), int(depth_imgs.shape[2])
        if tuple(rgb_imgs.shape) != (bsz, h, w, 3):
            raise ValueError(f"rgb_imgs must be [B,H,W,3], got {tuple(rgb_imgs.shape)}")
        if tuple(poses.shape) != (bsz, 4, 4) or tuple(K.shape) != (bsz, 3, 3):
            raise ValueError("poses must be [B,4,4] and K [B,3,3]")
        if lazy is None and (clip_feat_img.shape[0] != bsz or clip_feat_img.shape[1] < self.n_clip_feats):
            raise ValueError(f"feature map must be [B,D>={self.n_clip_feats},npy,npx], got {tuple(clip_feat_img.shape)}")
        if fshape[0] < self.n_clip_feats:
            raise ValueError(f"the backbone yields {fshape[0]} channels, the volume holds {self.n_clip_feats}")
        for t, name in ((depth_imgs, "depth_imgs"), (rgb_imgs, "rgb_imgs"), (poses, "poses"), (K, "K")) + (
                () if lazy is not None else ((clip_feat_img, "clip feature map"),)):
            require_cuda(t, name)
        if label_maps is not None:
            for m in label_maps:
                require_cuda(m, "label map")
                if tuple(m.shape) != (h, w):
                    raise ValueError("label map must be [H,W]")
        # frames queued together share the shapes and, for deferred features, the backbone call and its autocast state
        key = (h, w, tuple(fshape), label_maps is not None, bool(rgb_bilinear), None if lazy is None else (id(lazy[0]),) + lazy[1:])
        q = self.__dict__["_queue"]
        ring = q.ring
        if ring is None or ring.key != key:
            self._flush_pending(final=True)  # (the old ring's frames; the session of the old shape)
            ring = q.ring = StagingRing(key, lazy, self._QUEUE_FRAMES, self._buffers["tsdf"].device)
        q.stage(self, ring, depth_imgs, rgb_imgs, poses, K, clip_feat_img, label_maps,
                bool(self.__dict__.get("borrow_inputs", _BORROW_DEFAULT)))

    def flush(self):
        """Bring the registered buffers up to date: fuse the frames queued behind integrate() and finish a deferred
        clear (reset).  Readers of the volume never need to call it -- every access to a registered buffer does -- it
        exists for callers that hold raw pointers or tensors obtained earlier."""
        self._sync_volume()

    def _sync_volume(self):
        # the frames flushed HERE are the last before somebody looks: the queue's session is finished behind them, the deferred
        # clear of reset() -- still owed after the flushes the queue started on its own: a scan of several windows would otherwise
        # zero, after its first window, most of a volume that the later windows write -- is paid, and the current stream waits
        self._flush_pending(final=True)
        if self.__dict__.get("_feat_stale"):
            # reset() did not clear the feature rows: zero the ones that are still unwritten (weight 0)
            self.__dict__["_feat_stale"] = False
            vol = self._c_volume(for_fuse=True)
            dev = self._buffers["tsdf"].device
            with torch.cuda.device(dev):
                check(lib().saf_clear_unwritten_rows(C.byref(vol), 0, self._buffers["tsdf"].numel(), current_stream_ptr()),
                      "saf_clear_unwritten_rows")

    def _queue_busy(self):
        """Frames staged but not handed over, or a pushed window whose row kernel is still owed."""
        q = self.__dict__.get("_queue")
        return q is not None and q.busy()

    def _flush_pending(self, final=False, keep=0):
        """Hand the staged frames to the library.  ``final``: somebody is about to look -- the session is finished behind them
        (its last window's rows launched, the current stream waits); else the frames but the newest ``keep`` are pushed into
        the session (the newest chunk's staging and depth tiles are still running: it follows one chunk later, wait-free)."""
        q = self.__dict__.get("_queue")
        if q is None:
            return
        n = q.pending - (0 if final else keep)
        keep = q.pending - n
        if n <= 0:
            if final:
                q.finish_session(self)
            return
        self._check_poisoned()
        q.pending = 0  # first: the buffer accesses below must not re-enter
        q.launched = False
        ring = q.ring
        lo = ring.ring0
        sl = slice(lo, lo + n)
        try:
            labs = None if ring.labels is None else ring.labels[sl]
            feat = ring.feat[sl]
            if ring.lazy is not None:  # the queued frames' feature maps, in one backbone batch
                fn, ac_on, ac_dtype = ring.lazy
                with torch.no_grad(), torch.autocast("cuda", dtype=ac_dtype, enabled=ac_on):
                    feat = fn(ring.rgb[sl])
                if tuple(feat.shape) != (n,) + tuple(ring.key[2]):
                    raise SafError(f"the backbone returned {tuple(feat.shape)} for {n} frames, expected {(n,) + tuple(ring.key[2])}")
                # into the ring: the last window's row kernel reads its maps when the NEXT push launches it -- a temporary of
                # this call would be back in the allocator's hands by then (the ring's quarters are guarded by events)
                ring.feat[sl].copy_(feat)
                feat = ring.feat[sl]
            # (looked up on the instance at every flush: a test replaces it there)
            self._fuse_now(ring.depth[sl], ring.rgb[sl], ring.pose[sl], ring.K[sl], feat, labs, ring.key[4], staged=(lo, n, final))
        except BaseException as exc:
            if not q.launched:
                # the backbone, the descriptors or the argument checks at the entry of the fuse call failed (out of
                # memory, an unsupported tiling) BEFORE any kernel touched the volume: the frames stay queued -- the next
                # access raises again instead of reading a volume that silently lacks them
                q.pending = n + keep
            else:
                # the call failed after launching some of its windows: fusing the same frames again would count them
                # twice, dropping them would lose them silently.  Neither: the volume is unusable until reset().
                self.__dict__["_poisoned"] = f"a flush of {n} queued frames failed part-way ({exc!r}); the volume is incomplete: reset() it"
            raise
        q.pending = keep
        if final:
            q.finish_session(self)
            ring.ring0 = 0  # (every quarter now carries the event of the finish, or of the call on the current stream)
            ring.release_borrowed()  # lent images: read by now as far as this stream can tell -- let them go
        else:
            ring.ring0 = (lo + n) % self._QUEUE_FRAMES  # the next frames follow in the ring (a session's windows are its quarters)

    def _check_poisoned(self):
        msg = self.__dict__.get("_poisoned")
        if msg:
            raise SafError(msg)

    @property
    def pending_frames(self):
        """Frames staged behind integrate() and not yet handed to the fuse call (a completed window is handed over at once)."""
        q = self.__dict__.get("_queue")
        return 0 if q is None else q.pending

    def __getattr__(self, name):
        # registered buffers live in _buffers, so every read of one comes through here
        if name in _VOLUME_BUFFERS:
            if self.__dict__.get("_poisoned"):
                self._check_poisoned()
            q = self.__dict__.get("_queue")
            if name == "clip_feat" and self.__dict__.get("_feat_stale"):
                self._sync_volume()  # queued frames AND the deferred clear: the rows are about to be looked at
            elif q is None:
                pass
            elif q.pending or q.session_open:
                self._flush_pending(final=True)
            elif q.event is not None:
                q.wait(self)  # (a reader on another stream than the one that finished the session)
        return super().__getattr__(name)

    def __setattr__(self, name, value):
        if (name in _VOLUME_BUFFERS or name == "accum_mode") and (self._queue_busy() or self.__dict__.get("_feat_stale")):
            self._sync_volume()  # queued frames belong to the buffers / mode that were current when they were queued
        super().__setattr__(name, value)

    def _apply(self, fn, *args, **kwargs):  # .to() / .cuda() / .cpu() / .float()
        if self._queue_busy() or self.__dict__.get("_feat_stale"):
            self._sync_volume()
        q = self.__dict__.get("_queue")
        if q is not None:
            q.wait(self)
            q.close()  # the session, the queue's stream and the ring belong to the device the module leaves
        return super()._apply(fn, *args, **kwargs)

    def _save_to_state_dict(self, *args, **kwargs):
        self._sync_volume()
        return super()._save_to_state_dict(*args, **kwargs)

    def _load_from_state_dict(self, *args, **kwargs):
        self._sync_volume()
        out = super()._load_from_state_dict(*args, **kwargs)
        # The windowed path never reads the feature row of a voxel whose weight is 0 (such a row is zero by construction).  A
        # loaded state need not keep that promise: the rows of weight-0 voxels are zeroed at the next access (the deferred
        # clear of reset(): saf_clear_unwritten_rows), so the invariant is enforced, not assumed.
        self.__dict__["_feat_stale"] = True
        return out

    def named_buffers(self, *args, **kwargs):
        self._sync_volume()
        return super().named_buffers(*args, **kwargs)

    def _fuse_now(self, depth_imgs, rgb_imgs, poses, K, clip_feat_img, label_maps=None, rgb_bilinear=False, staged=None):
        """``staged`` = (first ring slot, frames, final): the frames lie in the queue's staging ring -- where the windowed
        two-stream path takes them they are PUSHED into the queue's session on its own stream (their last window's row kernel
        stays owed: ``FrameQueue.finish_session``); everything else is one call on the current stream, behind the session."""
        if getattr(self, "_shard_stripes", None) is not None:
            raise SafError(
                "this volume holds only its reduce-scattered voxel stripes "
                f"({len(self._shard_stripes)} of them) of a merged job; all_gather it (distributed.gather_shards, or "
                "merge_volumes(..., gather=True)) before fusing more frames"
            )
        q = self.__dict__["_queue"]
        arr, keep, npy, npx = self._make_frames(depth_imgs, rgb_imgs, poses, K, clip_feat_img, label_maps, rgb_bilinear,
                                                borrowed=None if staged is None else q.ring.bptr[staged[0]:staged[0] + staged[1]])
        vol = self._c_volume(for_fuse=True)
        ws = self._get_workspace(npy, npx, (int(depth_imgs.shape[1]), int(depth_imgs.shape[2])))
        L = lib()
        windowed = L.saf_fuse_path(C.byref(vol), arr, len(arr), ws.numel()) == 1
        # the module's device, not the caller's current one, owns the launch (and its current stream)
        dev = self._buffers["tsdf"].device
        win = _abi.SAF_WINDOW_FRAMES
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            # (a flush of a few frames with no window open takes the per-frame pipeline, as a direct call of that size does)
            if staged is not None and (q.session_open or len(arr) >= 16) and \
                    L.saf_fuse_session_ok(C.byref(vol), arr, len(arr), ws.numel()) == 1:
                q.push(self, vol, arr, ws, staged[0], staged[1], dev, stream)
                return
            # one call on the current stream: whatever the session still owes comes first
            q.finish_session(self)
            # after a lazy reset() the feature rows still hold the previous scan: the windowed path never reads a weight-0 row
            # (the clear stays owed until somebody looks: _sync_volume); the per-frame pipeline reads the rows it updates --
            # saf_fuse_frames_recycled zeroes the unwritten rows first
            stale = bool(self.__dict__.get("_feat_stale")) and not windowed
            if stale:
                rc = L.saf_fuse_frames_recycled(
                    C.byref(vol), arr, len(arr), ws.data_ptr(), ws.numel(), self._buffers["fuse_stats"].data_ptr(), None, stream.cuda_stream
                )
            else:
                rc = L.saf_fuse_frames(
                    C.byref(vol), arr, len(arr), ws.data_ptr(), ws.numel(), self._buffers["fuse_stats"].data_ptr(), stream.cuda_stream
                )
            if stale and rc == 0:  # (the recycled call: every weight-0 row is zero behind it)
                self.__dict__["_feat_stale"] = False
            q.launched = rc == 0 or rc == _abi.SAF_E_HIP
            check(rc, "saf_fuse_frames")
            if staged is not None:  # the ring's slots of these frames are read on this stream
                ev = stream.record_event()
                for quarter in range(staged[0] // win, (staged[0] + staged[1] - 1) // win + 1):
                    q.ring.free_ev[quarter] = ev
            # the launches are asynchronous: keep inputs alive until the stream has consumed them
            for t in keep[:5]:
                t.record_stream(stream)
            for t in keep[5] or ():
                t.record_stream(stream)

    # -- extensions (not in the reference) ---------------------------------------------------
    def reset(self, accum_mode=_abi.SAF_RUNNING_MEAN, lazy=True):
        """Back to the freshly constructed state: every volume buffer zero (the reference builds a new module per
        scan, clip_seem_fusion.py:291-302).  The counters of ``stats()`` go on counting over the scans of a module: a
        caller who wants them per scan zeroes ``fuse_stats``.  ``lazy``: the 4*D*N bytes of ``clip_feat`` are not cleared here -- a voxel
        with weight 0 has a zero row by contract and the windowed fuse path never reads such rows; the rows still
        unwritten are zeroed when something first looks (any buffer access, state_dict, the merge, flush())."""
        q = self.__dict__["_queue"]
        q.pending = 0  # frames still queued would be fused into a volume that is being discarded
        self.__dict__["_poisoned"] = None
        self.__dict__["_feat_stale"] = False
        b = self._buffers
        q.abandon(b["tsdf"].device)  # (the open window goes with the volume; this stream waits for what the queue's still runs)
        lazy = bool(lazy) and b["clip_feat"].is_cuda
        for name in ("rgb", "tsdf", "weight", "tsdf_weight", "labels_one_hot") + (() if lazy else ("clip_feat",)):
            t = b.get(name)
            if t is not None:
                t.zero_()
        super().__setattr__("accum_mode", accum_mode)
        self._shard_stripes = None
        self.__dict__["_shard_plans"] = None
        self.__dict__["_shard16"] = None  # (distributed.shard_features_16's copy of the rows that were just discarded)
        self.__dict__["_feat_stale"] = lazy

    def integrate_features(self, depth_imgs, rgb_imgs, poses, K, clip_feat_img, label_maps=None):
        """``integrate`` with the backbone outputs supplied by the caller (fuse-only entry used by
        the benchmark and the parity tests)."""
        self._fuse(depth_imgs, rgb_imgs, poses, K, clip_feat_img, label_maps, self._rgb_bilinear)

    # -- taking fused frames out again (not in the reference: its running means only ever grow) --------------------------------
    # What ``windowed=None`` means: the windowed removal for calls of this many frames or more (where ``saf_unfuse_path`` is 1),
    # the per-frame removal below it (None: never).  Measured on an MI355X (tools/measure_unfuse.py, profiles/r15/unfuse_rate.txt:
    # 256^3 x 512 f32, 640 x 480 frames): at 16 frames -- the smallest count the windowed entry takes, and the smallest measured --
    # 3.99 ms against 5.01 .. 5.45 ms for the per-frame removal, a margin of 1.0 ms over a spread of 0.44 ms; 2.5 x at 128 frames.
    _UNFUSE_WINDOWED_MIN_FRAMES = 16

    def _unfuse(self, depth_imgs, rgb_imgs, poses, K, clip_feat_img, label_maps, strict, windowed=None):
        """``saf_unfuse_frames`` (include/saf.h) behind everything handed to ``integrate()`` so far -- ``windowed=True``:
        ``saf_unfuse_frames_windowed``, refused with ``SafError`` where ``saf_unfuse_path`` is not 1.  Returns the two skip
        counters as they stood before the call (``strict``; a device sync) or None."""
        if getattr(self, "_shard_stripes", None) is not None:
            raise SafError(
                "this volume holds only its reduce-scattered voxel stripes of a merged job; all_gather it "
                "(distributed.gather_shards, or merge_volumes(..., gather=True)) before taking frames out of it"
            )
        if self._buffers["clip_feat"].dtype != torch.float32:
            raise SafError("frames are taken out of torch.float32 volumes only: a stored bf16 / fp16 mean carries 2^-9 / 2^-12 relative "
                           "rounding, which taking a frame out multiplies by about the voxel's count (DESIGN 4.17)")
        if self.accum_mode != _abi.SAF_RUNNING_MEAN:
            raise SafError("frames are taken out of running means only: a SAF_SUM volume belongs to the multi-rank job (DESIGN 4.17)")
        self._check_poisoned()
        # what flush() does: the frames still queued, the row kernel a session owes, a deferred clear -- the current stream waits
        self._sync_volume()
        arr, keep, npy, npx = self._make_frames(depth_imgs, rgb_imgs, poses, K, clip_feat_img, label_maps, self._rgb_bilinear)
        vol = self._c_volume(for_fuse=True)
        ws = self._get_workspace(npy, npx, (int(depth_imgs.shape[1]), int(depth_imgs.shape[2])))
        dev = self._buffers["tsdf"].device
        stats = self._buffers["fuse_stats"]
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            before = stats[13:15].tolist() if strict else None
            L = lib()
            takes = L.saf_unfuse_path(C.byref(vol), arr, len(arr), ws.numel()) == 1
            if windowed is None:
                floor = self._UNFUSE_WINDOWED_MIN_FRAMES
                windowed = takes and floor is not None and len(arr) >= floor
            if windowed and not takes:
                raise SafError("windowed=True: the windowed removal does not take this call (saf_unfuse_path, include/saf.h: f32 "
                               "running means of feat_dim 256 / 512 / 768 / 1024, 16 or more frames of one shape, SAF_WIN_FORM "
                               "unset or sums); windowed=False removes the frames through the per-frame pipeline")
            entry, name = (L.saf_unfuse_frames_windowed, "saf_unfuse_frames_windowed") if windowed else (L.saf_unfuse_frames, "saf_unfuse_frames")
            check(entry(C.byref(vol), arr, len(arr), ws.data_ptr(), ws.numel(), stats.data_ptr(), stream.cuda_stream), name)
            # the launches are asynchronous: keep inputs alive until the stream has consumed them
            for t in keep[:5]:
                t.record_stream(stream)
            for t in keep[5] or ():
                t.record_stream(stream)
        return before

    def _unfuse_strict(self, before):
        if before is not None:
            after = self._buffers["fuse_stats"][13:15].tolist()  # (synchronises)
            if after != before:
                raise SafError(f"de-integration skipped {after[0] - before[0]} valid and {after[1] - before[1]} tsdf-valid voxel updates "
                               "whose count was already 0: these frames were not fused under these poses")

    def deintegrate_features(self, depth_imgs, rgb_imgs, poses, K, clip_feat_img, label_maps=None, strict=False, windowed=None):
        """The mirror of ``integrate_features``: take these frames OUT of the volume again, given the inputs they were fused with
        (depth, pose and ``K`` decide which voxels a frame touches; rgb, feature and label maps what leaves them).  Frames still
        queued behind ``integrate()`` are fused first.  A voxel whose last frame leaves is zero again, bit for bit; every other
        running mean is within fp32 rounding of the mean without the frame.  A touched voxel whose count is already
        0 -- the frame was never fused, or under another pose -- is skipped and counted (``stats()["deintegrate_skipped"]``);
        ``strict=True`` synchronises and raises ``SafError`` if that happened during this call.  float32 running-mean volumes
        only; a voxel-sharded (striped) volume is refused.

        ``windowed``: ``False`` = the per-frame pipeline run backwards (every width and grid); ``True`` = the windowed removal
        (``saf_unfuse_frames_windowed``: every touched feature row read and written once per window of 128 frames -- counts, tsdf,
        rgb and histograms bit for bit the per-frame removal's, feature rows within fp32 rounding of it), ``SafError`` where it
        does not apply (f32 volumes of feat_dim 256 / 512 / 768 / 1024, calls of 16 or more frames of one shape); ``None`` = the
        windowed removal wherever it applies (from 16 frames it is the faster one: 1.3 x there, 2.5 x at 128 frames),
        the per-frame pipeline elsewhere."""
        self._unfuse_strict(self._unfuse(depth_imgs, rgb_imgs, poses, K, clip_feat_img, label_maps, strict, windowed))

    def reintegrate_features(self, depth_imgs, rgb_imgs, old_poses, new_poses, K, clip_feat_img, label_maps=None, strict=False,
                             windowed=None):
        """Move fused frames to corrected poses: ``deintegrate_features`` under ``old_poses``, ``integrate_features`` under
        ``new_poses``, with the same maps.  ``strict`` and ``windowed`` (the removal's path) as there; the frames are put back
        either way, by the path ``integrate_features`` takes."""
        before = self._unfuse(depth_imgs, rgb_imgs, old_poses, K, clip_feat_img, label_maps, strict, windowed)
        self._fuse(depth_imgs, rgb_imgs, new_poses, K, clip_feat_img, label_maps, self._rgb_bilinear)
        self._unfuse_strict(before)

    def deintegrate(self, depth_imgs, rgb_imgs, poses, K, strict=False, windowed=None):
        """The mirror of ``integrate``: the same backbone calls yield the feature (and label) maps, then ``deintegrate_features``."""
        feat, label_maps = self._frame_maps(depth_imgs, rgb_imgs, K)
        self.deintegrate_features(depth_imgs, rgb_imgs, poses, K, feat, label_maps, strict=strict, windowed=windowed)

    def reintegrate(self, depth_imgs, rgb_imgs, old_poses, new_poses, K, strict=False, windowed=None):
        """What a user of ``refine_pose`` calls when a pose is corrected after its frame was fused: the frames leave the volume
        under ``old_poses`` and enter it again under ``new_poses``.  The backbones run ONCE."""
        feat, label_maps = self._frame_maps(depth_imgs, rgb_imgs, K)
        self.reintegrate_features(depth_imgs, rgb_imgs, old_poses, new_poses, K, feat, label_maps, strict=strict, windowed=windowed)

    def stats(self):
        """dict of counters accumulated by the kernels (forces a device sync)."""
        s = self.fuse_stats.cpu().tolist()
        if s[4]:
            raise SafError(f"{s[4]} fuse workgroups timed out waiting for their frame's sweep; the volume is incomplete")
        # the form the windowed path takes for this volume NOW (environment, read per call by the library): results of two
        # runs are comparable bit for bit only under the same form
        form = os.environ.get("SAF_WIN_FORM", "sums")
        form = {"s": "sums", "r": "rows", "b": "bricks"}.get(form[:1], "sums")
        maps16 = {torch.bfloat16: "bf16", torch.float16: "fp16"}.get(self._buffers["clip_feat"].dtype)
        if form == "bricks" and maps16 == "fp16":
            form = "sums"  # the brick form does not take fp16 rows: such a request gets the default form
        if form == "sums" and maps16 is not None:
            form = "rows (SAF_WIN_MAPS16=0)" if os.environ.get("SAF_WIN_MAPS16", "1")[:1] == "0" else f"sums, {maps16} map images"
        # the windowed path's frame cull: (brick, frame) pairs tested / dropped by reason (include/saf.h, stats[8..12])
        cull = {"pairs": s[8], "behind": s[9], "far": s[10], "frustum": s[11], "occluded": s[12]}
        return {"valid": s[0], "tsdf_valid": s[1], "frames": s[2], "labels_dropped": s[3], "window_rows": s[5],
                "window_tsdf_voxels": s[6], "window_form": form, "cull": cull,
                "deintegrate_skipped": {"valid": s[13], "tsdf_valid": s[14]}}

    def sample_mesh_vertices(self, verts_index, voxel_obj_idx=None, objects_segmentation_color=None):
        """The sampling half of ``extract_mesh`` (reference clipfusion.py:741-760, clip_seem_fusion.py:843-878)
        on the HIP device: marching-cubes vertices in voxel-index coordinates -> (vertex_colors[V,3] clamped,
        vertex_clip_feats[V,D] f32[, vertex_obj_idx[V,1], vertex_segment_color[V,3]])."""
        verts = torch.as_tensor(np.asarray(verts_index, dtype=np.float32)).to(self.tsdf.device).contiguous()
        nv = verts.shape[0]
        dev = self.tsdf.device
        feat = torch.empty((nv, int(self.n_clip_feats)), dtype=torch.float32, device=dev)
        rgb = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        oi = so = oo = sc = None
        if voxel_obj_idx is not None:
            oi = torch.as_tensor(voxel_obj_idx).to(device=dev, dtype=torch.int32).contiguous().reshape(-1)
            oo = torch.empty(nv, dtype=torch.float32, device=dev)
        if objects_segmentation_color is not None:
            sc = self._f32c(torch.as_tensor(objects_segmentation_color).to(dev), "objects_segmentation_color")
            so = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        vol = self._c_volume()
        p = _abi.ptr
        with torch.cuda.device(dev):
            rc = lib().saf_sample_vertices(C.byref(vol), p(verts), nv, p(feat), p(rgb), p(oi), p(oo), p(sc), p(so),
                                           current_stream_ptr())
        check(rc, "saf_sample_vertices")
        out = [rgb, feat]
        if oo is not None:
            out.append(oo[:, None])
        if so is not None:
            out.append(so)
        return tuple(out)

    def _marching_cubes_vertices(self, marching_cubes=None):
        """TSDF -> (verts in index space, faces) (clipfusion.py:724-739): un-fused voxels act as NaN, faces touching
        a NaN vertex are dropped, vertices re-indexed.  Default: on the device (saf_marching_cubes_*), nothing but the
        mesh leaves it.  ``marching_cubes=`` takes a callable with scikit-image's signature (e.g.
        ``skimage.measure.marching_cubes``) to run the reference's own CPU route instead."""
        if marching_cubes is None:
            nx, ny, nz = (int(v) for v in self.nvox)
            verts, faces = marching_cubes_gpu(self.tsdf.view(nx, ny, nz), self.weight.view(nx, ny, nz), level=0.0)
            return verts.cpu().numpy(), faces.cpu().numpy().astype(np.int64)
        tsdf = self.tsdf.masked_fill(self.weight == 0, torch.nan).cpu()
        verts, faces = marching_cubes(tsdf.view(*[int(v) for v in self.nvox]).numpy(), level=0)[:2]
        faces = faces[~np.isnan(verts[faces]).any(axis=(1, 2))]
        used = np.zeros(len(verts), dtype=bool)
        used[np.unique(faces)] = True
        faces = (np.cumsum(used) - 1)[faces]
        return verts[used], faces

    def _verts_world(self, verts):
        if any(self.index_offset):  # a box that does not start at the lattice's voxel 0 (move_grid)
            verts = verts + np.asarray(self.index_offset, dtype=verts.dtype)
        return verts * self.voxel_size + torch.as_tensor(self.origin).cpu().numpy()

    def extract_mesh(self, marching_cubes=None):
        """Reference clipfusion.py:723-763: (verts_world, faces, vertex_colors, vertex_clip_feats).  Marching cubes
        and the vertex sampling of the D-channel volume both run in HIP; the volume never leaves the device."""
        verts, faces = self._marching_cubes_vertices(marching_cubes)
        colors, feats = self.sample_mesh_vertices(verts)[:2]
        return self._verts_world(verts), faces, colors, feats

    # -- viewing the volume from a pose (not in the reference: its AR client needs it, app_unity.py) --------------
    def render(self, pose, K, height, width, step_vox=0.5, z_near=0.0, z_far=None, rgb=True):
        """What a camera at ``pose`` (cam->world [4,4]) with intrinsics ``K`` [3,3] sees of the volume (saf_raycast, include/saf.h):
        a ``RenderResult`` of device tensors -- ``depth`` [H,W] f32 (camera z of the first front-face zero crossing of the TSDF,
        0 = miss), ``voxel`` [H,W] i32 (flat index of the voxel nearest to the hit, -1 = miss), ``rgb`` [H,W,3] f32 (that voxel's
        colour; None with ``rgb=False``) and ``hit`` (``voxel >= 0``).  ``step_vox``: sample spacing in voxels along the ray's
        dominant axis; ``z_far=None``: the grid's diagonal.  Frames still queued behind ``integrate()`` are fused first.

        Two things a caller should know.  A ``K`` with skew or a third row other than (0, 0, 1) is not supported: ``K`` lives on
        the device and is not read back, so no error is raised -- every pixel comes back as a miss.  And the answer is that of
        the fused FIELD: a camera outside the scanned room looks at the back of the walls' truncation bands, whose outer edge
        (carved to free space by oblique frames, left negative by head-on ones) can read as a surface -- tens of pixels of a
        view may report a depth just outside a wall.  A camera inside the scanned space never sees a band from behind."""
        pose = self._f32c(torch.as_tensor(pose), "pose")
        K = self._f32c(torch.as_tensor(K), "K")
        if tuple(pose.shape) != (4, 4) or tuple(K.shape) != (3, 3):
            raise ValueError("pose must be [4,4] and K [3,3]")
        if getattr(self, "_shard_stripes", None) is not None or self.x_planes is not None:
            raise SafError("render() needs the whole grid: this module holds a slab / the stripes of a voxel-sharded volume")
        vol = self._c_volume()  # (joins the queue: the volume holds every frame handed to integrate())
        dev = self._buffers["tsdf"].device
        height, width = int(height), int(width)
        if z_far is None:
            z_far = _grid_diagonal(self.voxel_size, self.nvox)
        shape = (max(height, 0), max(width, 0))
        depth = torch.empty(shape, dtype=torch.float32, device=dev)
        voxel = torch.empty(shape, dtype=torch.int32, device=dev)
        color = torch.empty(shape + (3,), dtype=torch.float32, device=dev) if rgb else None
        p = _abi.ptr
        with torch.cuda.device(dev):
            rc = lib().saf_raycast(C.byref(vol), p(pose.to(dev)), p(K.to(dev)), height, width, float(step_vox), float(z_near),
                                   float(z_far), p(depth), p(voxel), p(color), current_stream_ptr())
        check(rc, "saf_raycast")
        return RenderResult(depth=depth, voxel=voxel, rgb=color, hit=voxel >= 0)

    def render_query(self, text_features, pose, K, height, width, epilogue="softmax", scale=100.0, normalize=True, **render_kw):
        """``render`` plus ``relevance`` [H,W,L] f32: the text query of ``Clip.run_query`` (epilogue "softmax", or the raw
        "scores") over the feature rows of the voxels the pixels see -- saf_gather_rows on ``clip_feat``, then the scan every
        other query uses (fp32, bf16 and fp16 volumes).  Miss pixels get 0 in every column.  (Feature surgery weighs the labels over
        the whole row set: not offered per view.)"""
        epi = {"scores": _abi.SAF_Q_SCORES, "softmax": _abi.SAF_Q_SOFTMAX}.get(epilogue)
        if epi is None:
            raise ValueError(f"render_query takes the epilogues 'scores' and 'softmax', not {epilogue!r}")
        out = self.render(pose, K, height, width, **render_kw)
        rows = gather_rows(self.clip_feat, out.voxel.reshape(-1))
        text_features = torch.as_tensor(text_features)
        rel = _query_scan(rows, text_features, epi, scale=scale, normalize=normalize)
        rel = rel.masked_fill_(~out.hit.reshape(-1, 1), 0.0)
        out.relevance = rel.view(out.voxel.shape[0], out.voxel.shape[1], -1)
        return out

    # -- refining a camera pose against the volume (not in the reference: it fuses with the capture app's poses) ------------
    def refine_pose(self, depth, pose, K, levels=((4, 6), (2, 4), (1, 4)), huber=0.3, r_max=0.9, damping=1e-2, tol_t=None,
                    tol_r=None, min_valid=100, max_shift_t=None, max_shift_r=0.05):
        """The pose that puts a depth frame's points on the zero set of the fused TSDF (saf_pose_refine, include/saf.h): a fixed
        Gauss-Newton on the device, coarse to fine over ``levels`` = ((pixel stride, iterations), ...), started at ``pose``
        (cam->world [4,4]).  Returns a ``PoseRefinement`` of device tensors; nothing is read back until one of its properties is.
        ``depth`` [H,W] with ``pose`` [4,4], or [B,H,W] with [B,4,4] (``K`` [3,3] or [B,3,3]): the frames are refined one after the
        other against the same volume.  Frames still queued behind ``integrate()`` are fused first.

        ``huber`` and ``r_max`` are in units of the truncation distance, ``tol_t`` / ``max_shift_t`` in metres (defaults: 0.05
        voxel and the truncation distance), ``tol_r`` / ``max_shift_r`` in radians (default ``tol_r``: ``tol_t`` seen over a
        2.5 m lever).  A frame that cannot be refined -- fewer than ``min_valid`` pixels on observed voxels inside the band
        (status 2: an empty volume, a pose far off), a singular system (3), an unsupported ``K`` (4), a result farther from
        ``pose`` than the shift caps (5) -- comes back with its input pose, byte for byte; status 1 (iterations used up) returns
        the last iterate.  DESIGN 4.16 has the reasons for the defaults and what bounds the basin: the truncation band."""
        depth = self._f32c(torch.as_tensor(depth), "depth")
        pose = self._f32c(torch.as_tensor(pose), "pose")
        K = self._f32c(torch.as_tensor(K), "K")
        batched = depth.dim() == 3
        if not batched:
            depth, pose = depth[None], pose[None]
        if depth.dim() != 3 or tuple(pose.shape) != (depth.shape[0], 4, 4):
            raise ValueError("depth must be [H,W] with pose [4,4], or [B,H,W] with pose [B,4,4]")
        if K.dim() == 2:
            K = K[None].expand(depth.shape[0], 3, 3)
        if tuple(K.shape) != (depth.shape[0], 3, 3):
            raise ValueError("K must be [3,3] or [B,3,3]")
        if getattr(self, "_shard_stripes", None) is not None or self.x_planes is not None:
            raise SafError("refine_pose() needs the whole grid: this module holds a slab / the stripes of a voxel-sharded volume")
        levels = [(int(s), int(n)) for s, n in levels]
        vol = self._c_volume()  # (joins the queue: the volume holds every frame handed to integrate())
        dev = self._buffers["tsdf"].device
        depth, pose, K = depth.to(dev), pose.to(dev), K.contiguous().to(dev)
        b, height, width = (int(v) for v in depth.shape)
        vs = float(self.voxel_size)
        tol_t = 0.05 * vs if tol_t is None else float(tol_t)
        prm = _abi.SafPoseParams(float(huber), float(r_max), float(damping), tol_t, tol_t / 2.5 if tol_r is None else float(tol_r),
                                 int(min_valid), float(self.trunc) if max_shift_t is None else float(max_shift_t), float(max_shift_r))
        n_rows = sum(n for _, n in levels)
        strides = (C.c_int32 * len(levels))(*[s for s, _ in levels])
        iters = (C.c_int32 * len(levels))(*[n for _, n in levels])
        need = lib().saf_pose_workspace_bytes(height, width, min([s for s, _ in levels], default=0))
        ws = torch.empty(max(int(need), 1), dtype=torch.uint8, device=dev)
        out_pose = torch.empty((b, 4, 4), dtype=torch.float32, device=dev)
        out_log = torch.empty((b, max(n_rows, 0), 8), dtype=torch.float64, device=dev)
        out_status = torch.empty(b, dtype=torch.int32, device=dev)
        p = _abi.ptr
        with torch.cuda.device(dev):
            for i in range(b):
                rc = lib().saf_pose_refine(C.byref(vol), p(depth[i]), height, width, p(pose[i]), p(K[i]), strides, iters, len(levels),
                                           C.byref(prm), p(out_pose[i]), p(out_log[i]), p(out_status[i:i + 1]), p(ws), ws.numel(),
                                           current_stream_ptr())
                check(rc, "saf_pose_refine")
        if not batched:
            out_pose, out_log, out_status = out_pose[0], out_log[0], out_status[0]
        return PoseRefinement(pose=out_pose, log=out_log, status=out_status)

    def integrate_refined(self, depth_imgs, rgb_imgs, poses, K, **refine_kw):
        """``integrate`` with poses that drift: per frame, ``refine_pose`` against the volume as fused so far, then ``integrate``
        with the refined pose.  Returns the poses used, [B,4,4] on the device.  No host decision is taken: a frame that cannot be
        refined (an empty volume at the start of a scan, too few valid pixels, ...) is fused with its own pose by the kernel's
        rule.  Each frame's refinement reads the volume with every earlier frame in it, so this path gives up the deferred
        queue's overlap by construction: every frame is a flush."""
        poses = self._f32c(torch.as_tensor(poses), "poses")
        K = self._f32c(torch.as_tensor(K), "K")
        if K.dim() == 2:
            K = K[None].expand(poses.shape[0], 3, 3)
        used = []
        for i in range(int(poses.shape[0])):
            ref = self.refine_pose(depth_imgs[i], poses[i], K[i], **refine_kw)
            used.append(ref.pose)
            self.integrate(depth_imgs[i:i + 1], rgb_imgs[i:i + 1], ref.pose[None], K[i:i + 1])
        return torch.stack(used) if used else poses.new_zeros((0, 4, 4))


def _grid_diagonal(voxel_size, nvox):
    return float(voxel_size) * math.sqrt(sum(float(n) ** 2 for n in nvox))


@dataclass
class RenderResult:
    """What ``render`` / ``render_query`` return: per-pixel device tensors ([H,W,...]); fields a call does not produce are None."""

    depth: torch.Tensor
    voxel: torch.Tensor
    rgb: torch.Tensor | None
    hit: torch.Tensor
    label: torch.Tensor | None = None      # ClipSeemFusion.render: panoptic class of the voxel, -1 = miss
    relevance: torch.Tensor | None = None  # render_query: [H,W,L]


@dataclass
class PoseRefinement:
    """What ``refine_pose`` returns: device tensors (a leading batch dimension for a batched call).  ``log`` rows are
    [stride, n_valid, cost / n_valid, |v|, |omega|, status of the step, 0, 0]; rows never reached are zero.  The properties read
    the device (a synchronisation) only when they are asked."""

    pose: torch.Tensor    # [4,4] f32: the refined pose, or the input pose where status is 2 .. 5
    log: torch.Tensor     # [sum(iters), 8] f64
    status: torch.Tensor  # i32: 0 converged, 1 iterations used up, 2 too few valid pixels, 3 singular, 4 bad K, 5 shift cap

    def _last_row(self):
        log = self.log.cpu()
        reached = log[..., 0] > 0
        last = (reached.long().cumsum(-1) * reached).argmax(-1)
        row = torch.gather(log, -2, last[..., None, None].expand(*last.shape, 1, 8)).squeeze(-2)
        return row * reached.any(-1, keepdim=True)

    @property
    def converged(self):
        s = self.status.cpu() == 0
        return bool(s) if s.dim() == 0 else s

    @property
    def n_valid(self):
        r = self._last_row()[..., 1].long()
        return int(r) if r.dim() == 0 else r

    @property
    def cost(self):
        r = self._last_row()[..., 2]
        return float(r) if r.dim() == 0 else r


def gather_rows(src, index):
    """``out[p] = src[index[p]]``, rows of zeros where ``index[p] < 0`` (saf_gather_rows): ``src`` [N, ...] contiguous on the HIP
    device with rows of a multiple of 16 bytes, ``index`` [P] int32."""
    require_cuda(src, "the rows to gather")
    require_cuda(index, "the row index")
    if not src.is_contiguous():
        raise SafError("gather_rows needs contiguous rows")
    idx = index.to(device=src.device, dtype=torch.int32).contiguous().reshape(-1)
    n = int(src.shape[0])
    row_bytes = (src.numel() // max(n, 1)) * src.element_size()
    out = torch.empty((idx.numel(),) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    if idx.numel() == 0:
        return out
    with torch.cuda.device(src.device):
        rc = lib().saf_gather_rows(src.data_ptr(), n, row_bytes, idx.data_ptr(), idx.numel(), out.data_ptr(), current_stream_ptr())
    check(rc, "saf_gather_rows")
    return out


# --------------------------------------------------------------------------------------------
# Clip: tiled image features (PyTorch-ROCm backbone) + the text query head (HIP scan)
# --------------------------------------------------------------------------------------------


def _norm_mode(normalize):
    """False/0 -> none; True/1 -> L2 + nan_to_num (clip_seem_fusion.py:507-511); 2 / "clamp" -> divide by
    max(norm, 0.1) as eval_scannet_segmentation.py:549-551 and hypersim_eval.py:50-51 do."""
    if normalize in ("clamp", "clamp_min"):
        return _abi.SAF_NORM_L2_CLAMP
    if isinstance(normalize, bool):
        return int(normalize)
    mode = int(normalize)
    if mode not in (_abi.SAF_NORM_NONE, _abi.SAF_NORM_L2, _abi.SAF_NORM_L2_CLAMP):
        raise ValueError(f"bad normalize mode {normalize!r}")
    return mode


def _query_scan(feats, text, epilogue, scale=1.0, normalize=False, last_only=False):
    """Run saf_query_scan on [N,D] f32 features and [L,>=D] f32 text embeddings (both moved to the
    HIP device if needed); returns [N,L] (or [N] when last_only) on the device of ``feats``."""
    if not torch.cuda.is_available():
        raise SafError("the query scan needs the MI355X device; there is no CPU fallback")
    out_dev = feats.device
    dev = feats.device if feats.is_cuda else torch.device("cuda", torch.cuda.current_device())
    f = feats.detach().to(device=dev)
    ft = {torch.float32: _abi.SAF_F32, torch.bfloat16: _abi.SAF_BF16, torch.float16: _abi.SAF_F16}.get(f.dtype)
    if ft is None:
        f, ft = f.float(), _abi.SAF_F32
    if f.dim() != 2:
        raise ValueError("features must be [N,D]")
    if f.stride(1) != 1:
        f = f.contiguous()
    t = text.detach().to(device=dev, dtype=torch.float32)
    if t.stride(1) != 1:
        t = t.contiguous()
    n, d = f.shape
    nl = t.shape[0]
    if t.shape[1] < d:
        raise RuntimeError(f"text features have {t.shape[1]} dims, image features {d}")
    out = None if last_only else torch.empty((n, nl), dtype=torch.float32, device=dev)
    last = torch.empty(n, dtype=torch.float32, device=dev) if last_only else None
    wsb = lib().saf_query_workspace_bytes(nl, epilogue)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev) if wsb else None
    with torch.cuda.device(dev):
        rc = lib().saf_query_scan(
            f.data_ptr(), ft, n, f.stride(0), d, t.data_ptr(), nl, t.stride(0), epilogue, float(scale),
            _norm_mode(normalize), _abi.ptr(out), _abi.ptr(last), _abi.ptr(ws), wsb, current_stream_ptr(),
        )
    check(rc, "saf_query_scan")
    res = last if last_only else out
    return res.to(out_dev)


def marching_cubes_gpu(tsdf, weight, level=0.0):
    """Marching cubes on the device (saf_marching_cubes_count / _emit): ``tsdf`` [nx,ny,nz] f32 and ``weight`` [nx,ny,nz]
    i32 on the HIP device -> (verts [V,3] f32 in voxel-index coordinates, faces [F,3] i32), both on the device.
    Voxels with weight 0 are the reference's NaN mask (clipfusion.py:724); faces with a vertex on an edge to such a
    voxel do not exist, nor do unused vertices (clipfusion.py:730-739)."""
    require_cuda(tsdf, "tsdf")
    require_cuda(weight, "weight")
    if tsdf.dim() != 3 or tuple(weight.shape) != tuple(tsdf.shape):
        raise ValueError("tsdf and weight must be [nx,ny,nz]")
    t = tsdf.float().contiguous()
    w = weight.to(torch.int32).contiguous()
    nx, ny, nz = (int(v) for v in t.shape)
    dev = t.device
    L = lib()
    if min(nx, ny, nz) < 2:
        return torch.zeros((0, 3), device=dev), torch.zeros((0, 3), dtype=torch.int32, device=dev)
    wsb = L.saf_marching_cubes_workspace_bytes(nx * ny * nz)
    if wsb == 0:
        raise SafError("marching cubes: the grid is too large (2^31 voxels or more)")
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(L.saf_marching_cubes_count(t.data_ptr(), w.data_ptr(), nx, ny, nz, float(level), ws.data_ptr(), wsb,
                                         counts.data_ptr(), current_stream_ptr()), "saf_marching_cubes_count")
        nv, nf = (int(v) for v in counts.tolist())  # the sizes are results: one read-back
        verts = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
        check(L.saf_marching_cubes_emit(t.data_ptr(), w.data_ptr(), nx, ny, nz, float(level), ws.data_ptr(), wsb,
                                        _abi.ptr(verts) if nv else None, nv, _abi.ptr(faces) if nf else None, nf,
                                        current_stream_ptr()), "saf_marching_cubes_emit")
    return verts, faces


_WIDE_EPILOGUES = {"scores": _abi.SAF_QW_SCORES, "vs_background": _abi.SAF_QW_VS_BACKGROUND,
                   "row_argmax": _abi.SAF_QW_ROW_ARGMAX, "query_max": _abi.SAF_QW_QUERY_MAX}


def query_scan_wide(feats, text, epilogue="scores", scale=1.0, normalize=True, n_background=0, rescale=False,
                    out_dtype=None, row_offset=0, out=None):
    """Many text queries over a 16-bit feature volume on the 16-bit matrix cores (BASELINE config 5: the
    query_mesh.py / hypersim_eval.py scan with ~1000 targets), with the callers' reductions fused into the scan
    (saf_query_scan_wide_ex) so that the N x Q score matrix -- twice the size of the volume -- need not exist.

    ``feats`` [N, D] float16 / bfloat16 on the HIP device, D in {256, 512} (128: scores only); ``text`` [Q, >=D] fp32
    (rounded to the feature dtype).  ``epilogue``:

    * ``"scores"``         -> [N, Q]: ``scale * <f_n / |f_n|, t_q>``
    * ``"vs_background"``  -> [N, Q - n_background]: ``softmax(scale * [<f, bg_0..>, <f, target>])[-1]`` for every target,
      the first ``n_background`` text rows being the shared background prompts (query_mesh.py:36-39 with
      ``scale=100``; hypersim_eval.py:76-81); ``rescale=True`` adds ``((r - 0.5) * 2).clamp(0, 1)`` (query_mesh.py:39)
    * ``"row_argmax"``     -> (index int32 [N], value f32 [N]): best query per row
      (eval_scannet_segmentation.py:553-560, the first label of the argsort)
    * ``"query_max"``      -> (value f32 [Q], row int64 [Q]): best row per query, rows numbered from ``row_offset``

    ``out``: an optional preallocated [N, columns] tensor for the two matrix-valued epilogues, a view at any row stride and
    base (row stride a multiple of 8 elements on a 16-byte base keeps the 16-byte stores of the epilogue; a multiple of 128 bytes
    is 3-4 % faster at many columns); only its own elements are written.  Rows with inf / NaN in them: include/saf.h,
    saf_query_scan_wide_ex.
    """
    require_cuda(feats, "features")
    if feats.dtype not in (torch.float16, torch.bfloat16) or feats.dim() != 2:
        raise ValueError("query_scan_wide needs a [N, D] float16 / bfloat16 feature tensor")
    if feats.stride(1) != 1:
        feats = feats.contiguous()
    epi = _WIDE_EPILOGUES[epilogue] if isinstance(epilogue, str) else int(epilogue)
    out_dtype = out_dtype or feats.dtype
    dev = feats.device
    t = text.detach().to(device=dev, dtype=torch.float32)
    if t.stride(1) != 1:
        t = t.contiguous()
    n, d = feats.shape
    q = t.shape[0]
    if t.shape[1] < d:
        raise RuntimeError(f"text features have {t.shape[1]} dims, image features {d}")
    L = lib()
    norm = _norm_mode(normalize)
    if d == 128 and epi == _abi.SAF_QW_SCORES:  # the narrow shape keeps the first kernel
        if out is None:
            out = torch.empty((n, q), dtype=out_dtype, device=dev)
        else:
            require_cuda(out, "out")
            if tuple(out.shape) != (n, q) or out.stride(1) != 1:
                raise ValueError(f"out must be [{n}, {q}] with unit column stride")
            out_dtype = out.dtype
        wsb = L.saf_query_wide_workspace_bytes(q, d)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            rc = L.saf_query_scan_wide(feats.data_ptr(), _DT[feats.dtype], n, feats.stride(0), d, t.data_ptr(), q,
                                       t.stride(0), float(scale), norm, out.data_ptr(), _DT[out_dtype], out.stride(0),
                                       ws.data_ptr(), wsb, current_stream_ptr())
        check(rc, "saf_query_scan_wide")
        return out
    idx = val = row = None
    if epi in (_abi.SAF_QW_SCORES, _abi.SAF_QW_VS_BACKGROUND):
        cols = q - (int(n_background) if epi == _abi.SAF_QW_VS_BACKGROUND else 0)
        if out is None:
            # rows padded to a multiple of 8 columns keep every 16-byte store of the epilogue aligned; wide outputs are padded to
            # whole 128-byte lines (a tile's 64-byte segment then never straddles two lines: 3-4 % of the scan at 1000 columns,
            # tools/probe_out_stride.py).  The result is the [:, :cols] view
            esz = torch.empty((), dtype=out_dtype).element_size()
            per_line = 128 // esz
            stride = (cols + per_line - 1) // per_line * per_line if cols >= 4 * per_line else (cols + 7) // 8 * 8
            out = torch.empty((n, stride), dtype=out_dtype, device=dev)[:, :cols]
        else:
            require_cuda(out, "out")
            if tuple(out.shape) != (n, cols) or out.stride(1) != 1:
                raise ValueError(f"out must be [{n}, {cols}] with unit column stride")
            out_dtype = out.dtype
    elif epi == _abi.SAF_QW_ROW_ARGMAX:
        out = None
        idx = torch.empty(n, dtype=torch.int32, device=dev)
        val = torch.empty(n, dtype=torch.float32, device=dev)
    else:
        out = None
        val = torch.empty(q, dtype=torch.float32, device=dev)
        row = torch.empty(q, dtype=torch.int64, device=dev)
    wsb = L.saf_query_wide_ex_workspace_bytes(q, d, epi, int(n_background))
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = L.saf_query_scan_wide_ex(
            feats.data_ptr(), _DT[feats.dtype], n, feats.stride(0), d, t.data_ptr(), q, t.stride(0), float(scale), norm,
            epi, int(n_background), int(bool(rescale)), _abi.ptr(out), _DT[out_dtype], 0 if out is None else out.stride(0),
            _abi.ptr(idx), _abi.ptr(val), _abi.ptr(row), int(row_offset), ws.data_ptr(), ws.numel(), current_stream_ptr(),
        )
    check(rc, "saf_query_scan_wide_ex")
    if out is not None:
        return out
    return (idx, val) if idx is not None else (val, row)


def query_scores_wide(feats, text, scale=1.0, normalize=True, out_dtype=None):
    """Cosine scores of many text queries over a 16-bit feature volume: ``out[n, q] = scale * <f_n / |f_n|, t_q>``
    ([N, Q] of ``out_dtype``, default feats.dtype).  See query_scan_wide for the fused reductions."""
    return query_scan_wide(feats, text, "scores", scale=scale, normalize=normalize, out_dtype=out_dtype)


class Clip(torch.nn.Module):
    """Mirror of the reference ``Clip`` (clipfusion.py:766-1039).

    ``backbone``/``tokenizer`` may be injected (any object with ``encode_image``, ``encode_text``
    and ``visual.output_dim``); by default they come from ``open_clip`` exactly as in the
    reference (clipfusion.py:769-772).  The ViT GEMMs stay PyTorch-ROCm (hipBLASLt / MFMA).
    """

    # tiles per encode_image call.  The reference caps at 8 (clipfusion.py:826, sized for a 24 GB card); with 288 GB of HBM
    # the ViT GEMMs are fed 1024 tiles at a time: 468 -> 870-1000 frames/s end to end with a bf16 ViT-B/32 (bench.py --end-to-end)
    max_patch_batch_size = 1024

    def __init__(self, clip_model, pretraining, backbone=None, tokenizer=None):
        super().__init__()
        if backbone is None:
            try:
                import open_clip
            except ImportError as e:  # same failure mode as the reference's module import
                raise ImportError(
                    "open_clip is required to build the CLIP backbone (or pass backbone=/tokenizer=)"
                ) from e
            backbone = open_clip.create_model(clip_model, pretrained=pretraining, require_pretrained=True)
            tokenizer = open_clip.get_tokenizer(clip_model)
        self.clip = backbone
        self.tokenizer = tokenizer
        self.channel_mean = torch.nn.Parameter(
            torch.tensor([0.48145466, 0.4578275, 0.40821073])[None, :, None, None], requires_grad=False
        )
        self.channel_std = torch.nn.Parameter(
            torch.tensor([0.26862954, 0.26130258, 0.27577711])[None, :, None, None], requires_grad=False
        )
        self.feature_dim = self.clip.visual.output_dim

    def normalize_img(self, rgb_img_0_1):
        return (rgb_img_0_1 - self.channel_mean) / self.channel_std

    def unnormalize_img(self, rgb_img_normed):
        return rgb_img_normed * self.channel_std + self.channel_mean

    def get_patches(self, rgb_imgs, patch_size, patch_stride):
        """[B,3,H,W] -> [B,npy,npx,3,p,p] overlapping tiles (clipfusion.py:789-806)."""
        _, _, imheight, imwidth = rgb_imgs.shape
        assert (imheight - patch_size) % patch_stride == 0
        assert (imwidth - patch_size) % patch_stride == 0
        tiles = rgb_imgs.unfold(2, patch_size, patch_stride).unfold(3, patch_size, patch_stride)
        return tiles.permute(0, 2, 3, 1, 4, 5)

    def tiles_224(self, rgb_imgs, patch_size, patch_stride, dtype=None):
        """[B,3,H,W] in 0..1 -> the [B*npy*npx, 3, 224, 224] batch the ViT consumes (clipfusion.py:808-823: normalise,
        unfold, resize).  On the HIP device one fused kernel (saf_clip_tiles) writes it once, in ``dtype`` (default:
        the autocast dtype when autocast is on, else fp32); on the CPU the reference's three PyTorch steps."""
        _, _, imheight, imwidth = rgb_imgs.shape
        assert (imheight - patch_size) % patch_stride == 0
        assert (imwidth - patch_size) % patch_stride == 0
        if not rgb_imgs.is_cuda:
            patches = self.get_patches(self.normalize_img(rgb_imgs), patch_size, patch_stride)
            bsz, npy, npx = patches.shape[:3]
            patches = patches.reshape(bsz * npy * npx, 3, patch_size, patch_size)
            return torch.nn.functional.interpolate(patches, size=(224, 224), mode="bilinear", align_corners=False)
        if dtype is None:
            dtype = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else torch.float32
        x = rgb_imgs if rgb_imgs.dtype == torch.float32 else rgb_imgs.float()
        bsz = x.shape[0]
        npy, npx = 1 + (imheight - patch_size) // patch_stride, 1 + (imwidth - patch_size) // patch_stride
        out = torch.empty((bsz * npy * npx, 3, 224, 224), dtype=dtype, device=x.device)
        mean = (C.c_float * 3)(*self.channel_mean.detach().reshape(-1).tolist())
        std = (C.c_float * 3)(*self.channel_std.detach().reshape(-1).tolist())
        sb, sc, sy, sx = x.stride()
        with torch.cuda.device(x.device):
            rc = lib().saf_clip_tiles(x.data_ptr(), bsz, imheight, imwidth, sb, sc, sy, sx, int(patch_size), int(patch_stride),
                                      224, mean, std, out.data_ptr(), _DT[dtype], current_stream_ptr())
        check(rc, "saf_clip_tiles")
        return out

    def img_inference_tiled(self, rgb_imgs, patch_size, patch_stride):
        """[B,3,H,W] in 0..1 -> [B,D,npy,npx] CLIP embedding per tile (clipfusion.py:808-839)."""
        bsz = rgb_imgs.shape[0]
        npy = 1 + (rgb_imgs.shape[2] - patch_size) // patch_stride
        npx = 1 + (rgb_imgs.shape[3] - patch_size) // patch_stride
        per_frame = npy * npx
        feats = torch.empty(bsz * per_frame, self.feature_dim, device=rgb_imgs.device)
        step = int(self.max_patch_batch_size)
        # The tile batch is produced in slices of whole frames -- at most max_patch_batch_size tiles (and never more than the
        # tile kernel's 65535 per launch) exist at a time: the deferred-backbone queue hands over up to 512 frames at once,
        # whose tiles would be tens of GB (a fine tiling has hundreds of tiles per frame).
        fpb = max(1, min(step, 65535) // per_frame)
        for f0 in range(0, bsz, fpb):
            patches = self.tiles_224(rgb_imgs[f0 : f0 + fpb], patch_size, patch_stride)
            base = f0 * per_frame
            for start in range(0, len(patches), step):
                cur = patches[start : start + step]
                feats[base + start : base + start + len(cur)] = self.clip.encode_image(cur)
        return feats.view(bsz, npy, npx, self.feature_dim).permute(0, 3, 1, 2)

    def img_inference_tiled_depthscaled(self, rgb_imgs, depth_imgs, K, patch_stride, footprint_m=0.5):
        """[B,3,H,W] in 0..1, depth [B,H,W] m, K [B,3,3] -> [B,D,H,W]: a FULL-resolution feature image (clipfusion.py:841-890;
        ``scale_patches_by_depth``, off everywhere in the reference: :1097, clip_seem_fusion.py:167).  One tile per lattice
        point (every ``patch_stride`` pixels, the first row / column excluded) with a valid depth, sized to cover
        ``footprint_m`` metres at that depth (``round(f * 0.5 / depth)`` pixels, halves rounded down on both sides, clipped at
        the image's upper-left border only -- as the reference slices), resized to 224 x 224 and encoded; every pixel gets the
        MEAN of the embeddings of the tiles that cover it, 0 where none does.  All of an image's tiles go through the ViT in
        batches of ``max_patch_batch_size`` (the reference encodes them one by one).  The reference itself only runs for
        B = 1 (its last line divides [B, D, H, W] by [B, H, W]); any B works here."""
        x = self.normalize_img(rgb_imgs)
        bsz, _, h, w = x.shape
        dev = x.device
        ys = torch.arange(patch_stride, h, patch_stride, device=dev)
        xs = torch.arange(patch_stride, w, patch_stride, device=dev)
        out = torch.zeros(bsz, self.feature_dim, h, w, device=dev)
        step = int(self.max_patch_batch_size)
        for b in range(bsz):
            d = depth_imgs[b][ys][:, xs]                      # depth at the lattice points [ny, nx]
            keep = (d > 0).nonzero()
            if keep.numel() == 0:
                continue
            dk = d[keep[:, 0], keep[:, 1]]
            half_h = ((K[b, 1, 1] * footprint_m / dk).round().to(torch.int64) // 2).tolist()
            half_w = ((K[b, 0, 0] * footprint_m / dk).round().to(torch.int64) // 2).tolist()
            yc, xc = ys[keep[:, 0]].tolist(), xs[keep[:, 1]].tolist()
            boxes = [(max(0, y - hh), min(h, y + hh), max(0, x_ - hw), min(w, x_ + hw))
                     for y, x_, hh, hw in zip(yc, xc, half_h, half_w)]
            if any(y1 <= y0 or x1 <= x0 for y0, y1, x0, x1 in boxes):
                raise ValueError("a depth-scaled tile is empty (depth too large for this focal length); the reference's "
                                 "interpolate call raises for it as well")
            tiles = torch.cat([F.interpolate(x[b : b + 1, :, y0:y1, x0:x1], size=(224, 224), mode="bilinear", align_corners=False)
                               for y0, y1, x0, x1 in boxes])
            emb = torch.cat([self.clip.encode_image(tiles[s0 : s0 + step]) for s0 in range(0, len(tiles), step)]).to(out.dtype)
            cover = torch.zeros(h, w, device=dev)
            for (y0, y1, x0, x1), e in zip(boxes, emb):     # lattice order: the reference's order of additions
                out[b, :, y0:y1, x0:x1] += e[:, None, None]
                cover[y0:y1, x0:x1] += 1
            out[b] /= cover + (cover == 0)
        return out

    def text_inference(self, str_list):
        device = next(self.clip.parameters()).device
        tokens = self.tokenizer(str_list).to(device)
        feats = self.clip.encode_text(tokens)
        return feats / feats.norm(dim=-1, keepdim=True)

    def run_query(self, img_feats, labels):
        """softmax(100 * F @ T^T) over the labels (clipfusion.py:899-904), fused on the GPU."""
        d = img_feats.shape[-1]
        text = self.text_inference(labels)[:, :d]
        flat = img_feats.reshape(-1, d)
        rel = _query_scan(flat, text, _abi.SAF_Q_SOFTMAX, scale=100.0)
        return rel.reshape(*img_feats.shape[:-1], text.shape[0])

    @staticmethod
    def clip_feature_surgery(image_features, text_features, redundant_feats=None, t=2):
        """[b,n,c] x [t,c] -> [b,n,t] (clipfusion.py:906-934) without the [b,n,t,c] temporary."""
        if image_features.dim() != 3:
            raise ValueError("image_features must be [b,n,c]")
        if redundant_feats is not None:
            text = text_features - redundant_feats.to(text_features.device)
            return torch.stack([_query_scan(f, text, _abi.SAF_Q_SCORES) for f in image_features])
        if image_features.shape[0] != 1:
            # the reference's `w.reshape(1, 1, n_t, 1)` only works for b == 1
            raise RuntimeError("clip_feature_surgery without redundant_feats needs a batch of 1")
        return _query_scan(image_features[0], text_features, _abi.SAF_Q_SURGERY)[None]

    def encode_text_with_prompt_ensemble(self, texts, device, prompt_templates=None):
        """Mean of L2-normalised prompt embeddings per class, renormalised (clipfusion.py:936-1039)."""
        if prompt_templates is None:
            prompt_templates = IMAGENET_PROMPT_TEMPLATES
        model_device = next(self.clip.parameters()).device
        feats = []
        for text in texts:
            tokens = self.tokenizer([tpl.format(text) for tpl in prompt_templates])
            emb = self.clip.encode_text(tokens.to(model_device))
            emb = emb / emb.norm(dim=-1, keepdim=True)
            emb = emb.mean(dim=0)
            feats.append(emb / emb.norm())
        return torch.stack(feats, dim=0).to(device)


def _imagenet_templates():
    """The 85 prompt templates the reference uses by default (OpenAI's ImageNet prompt-engineering
    set plus five '... in the scene.' scene prompts, clipfusion.py:939-1025), generated from their
    regular structure rather than listed."""
    a_the = lambda pat: [pat.format(art) for art in ("a", "the")]
    singles = [
        "a photo of many {}.", "a photo of my {}.", "a photo of one {}.", "itap of my {}.",
        "there is a {} in the scene.", "there is the {} in the scene.", "this is a {} in the scene.",
        "this is the {} in the scene.", "this is one {} in the scene.",
    ]
    paired = [
        "a bad photo of {} {{}}.", "a sculpture of {} {{}}.", "a photo of {} hard to see {{}}.",
        "a low resolution photo of {} {{}}.", "a rendering of {} {{}}.", "graffiti of {} {{}}.",
        "a cropped photo of {} {{}}.", "a tattoo of {} {{}}.", "{} embroidered {{}}.",
        "a bright photo of {} {{}}.", "a photo of {} clean {{}}.", "a photo of {} dirty {{}}.",
        "a dark photo of {} {{}}.", "a drawing of {} {{}}.", "{} plastic {{}}.", "a photo of {} cool {{}}.",
        "a close-up photo of {} {{}}.", "a black and white photo of {} {{}}.", "a painting of {} {{}}.",
        "a pixelated photo of {} {{}}.", "a jpeg corrupted photo of {} {{}}.", "a blurry photo of {} {{}}.",
        "a photo of {} {{}}.", "a good photo of {} {{}}.", "{} {{}} in a video game.", "a doodle of {} {{}}.",
        "{} origami {{}}.", "a sketch of {} {{}}.", "{} toy {{}}.", "a rendition of {} {{}}.",
        "a photo of {} large {{}}.", "a photo of {} nice {{}}.", "a photo of {} weird {{}}.", "{} cartoon {{}}.",
        "art of {} {{}}.", "{} plushie {{}}.", "a photo of {} small {{}}.", "itap of {} {{}}.",
    ]
    out = list(singles)
    for pat in paired:
        out.extend(a_the(pat))
    return out


IMAGENET_PROMPT_TEMPLATES = _imagenet_templates()


# --------------------------------------------------------------------------------------------
# ClipFusion
# --------------------------------------------------------------------------------------------


def _lazy_clip_features(fusion, rgb_imgs):
    """(fn, (C, npy, npx)) if the CLIP feature maps of ``rgb_imgs`` [B,H,W,3] may be computed later, in one backbone batch
    with the other frames queued behind ``integrate()``: only for this package's own ``Clip`` (a pure function of the image;
    an injected object may depend on when it is called), and only if the tiling fits (else the call raises now, as the
    reference does).  ``defer_backbone=False`` in the constructor switches it off."""
    clip = fusion.clip
    if not isinstance(clip, Clip) or not fusion.__dict__.get("defer_backbone", True) or not fusion.__dict__.get("defer_frames", True):
        return None
    ps, stride = int(fusion.clip_patch_size), int(fusion.clip_patch_stride)
    h, w = int(rgb_imgs.shape[1]), int(rgb_imgs.shape[2])
    if rgb_imgs.dim() != 4 or h < ps or w < ps or (h - ps) % stride != 0 or (w - ps) % stride != 0:
        return None
    fn = fusion.__dict__.get("_lazy_fn")
    if fn is None or fn[1:] != (ps, stride, id(clip)):
        f = lambda rgb_nhwc: clip.img_inference_tiled(rgb_nhwc.permute(0, 3, 1, 2), patch_size=ps, patch_stride=stride)
        fn = (f, ps, stride, id(clip))
        fusion.__dict__["_lazy_fn"] = fn  # one function object per configuration: the queue's key compares its id
    return fn[0], (int(clip.feature_dim), 1 + (h - ps) // stride, 1 + (w - ps) // stride)


class ClipFusion(_FusionVolumeMixin, torch.nn.Module):
    """Dense voxel volume with projective running-average fusion (reference clipfusion.py:575-763).

    Constructor, attributes and registered buffer names follow the reference; ``integrate`` runs
    the hand-written HIP path (include/saf.h: saf_fuse_frames).  ``clip`` may be passed as a ready
    ``Clip``-like object through ``clip_model`` (anything with ``feature_dim`` and
    ``img_inference_tiled``), which is how tests and the benchmark inject seeded feature maps.
    """

    _rgb_bilinear = False  # nearest rgb sampling (clipfusion.py:701-706)

    def __init__(self, origin, voxel_size, nvox, trunc, scale_patches_by_depth, clip_model, clip_pretraining,
                 clip_patch_size, clip_patch_stride, keep_xyz_world=True, feat_dtype=torch.float32, defer_frames=True,
                 index_offset=(0, 0, 0), x_planes=None, defer_backbone=True, device=None):
        super().__init__()
        self.__dict__["defer_frames"] = bool(defer_frames)
        self.__dict__["defer_backbone"] = bool(defer_backbone)
        if isinstance(clip_model, str):
            self.clip = Clip(clip_model, clip_pretraining)
            self.clip.requires_grad_(False)
            self.clip.eval()
        else:
            self.clip = clip_model
        self.clip_patch_size = clip_patch_size
        self.clip_patch_stride = clip_patch_stride
        self.scale_patches_by_depth = scale_patches_by_depth
        self._init_volume(origin, voxel_size, nvox, trunc, self.clip.feature_dim, 0, keep_xyz_world, feat_dtype, index_offset,
                          x_planes, device)

    def integrate(self, depth_imgs, rgb_imgs, poses, K):
        """Fuse a batch of frames (reference clipfusion.py:627-721).  Batch elements are folded in
        one after the other; for B > 1 the reference updates the TSDF jointly over the batch
        (:681-695), which is the same mean up to fp32 rounding."""
        if not self.scale_patches_by_depth:
            lazy = _lazy_clip_features(self, rgb_imgs)
            if lazy is not None:
                return self._fuse(depth_imgs, rgb_imgs, poses, K, None, None, False, lazy_feat=lazy)
        clip_feat_img, _ = self._frame_maps(depth_imgs, rgb_imgs, K)
        self._fuse(depth_imgs, rgb_imgs, poses, K, clip_feat_img, None, False)

    def _frame_maps(self, depth_imgs, rgb_imgs, K):
        """The backbone call of ``integrate``: (feature maps, None) -- shared with ``deintegrate`` / ``reintegrate``."""
        if self.scale_patches_by_depth:
            return self.clip.img_inference_tiled_depthscaled(
                rgb_imgs.permute(0, 3, 1, 2), depth_imgs, K, patch_stride=self.clip_patch_stride
            ), None
        return self.clip.img_inference_tiled(
            rgb_imgs.permute(0, 3, 1, 2), patch_size=self.clip_patch_size, patch_stride=self.clip_patch_stride
        ), None


# --------------------------------------------------------------------------------------------
# backproject_pcd / bounds
# --------------------------------------------------------------------------------------------


def get_pix_vecs(imwidth, imheight, K):
    """Ray direction K^-1 [u,v,1]^T of every pixel, [B,H*W,3] (reference clipfusion.py:497-507).
    Kept for API compatibility; backproject_pcd below evaluates only the 7x7 lattice on the GPU."""
    v, u = torch.meshgrid(
        torch.arange(imheight, dtype=torch.float32, device=K.device),
        torch.arange(imwidth, dtype=torch.float32, device=K.device),
        indexing="ij",
    )
    uv1 = torch.stack((u, v, torch.ones_like(u)), dim=0).reshape(3, -1)
    return (K.inverse() @ uv1).transpose(1, 2)


def backproject_pcd(dataset, batch_size=1, num_workers=0, device="cpu", max_depth=torch.inf):
    """Sparse world-space point cloud of a scan: a 7x7 pixel lattice per frame un-projected with
    its depth (reference clipfusion.py:510-572).  The per-frame arithmetic runs in
    saf_backproject_lattice on the HIP device; ``device`` only says where the frames are staged
    in the reference and is accepted for compatibility.  Returns (xyz[M,3], rgb[M,3]) on the CPU."""
    if not torch.cuda.is_available():
        raise SafError("backproject_pcd needs the MI355X device; there is no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device())
    loader = torch.utils.data.DataLoader(dataset, batch_size=batch_size, num_workers=num_workers)
    uv_size = 7
    u = torch.round(torch.linspace(0, dataset.imwidth - 1, uv_size)).to(torch.int32)
    v = torch.round(torch.linspace(0, dataset.imheight - 1, uv_size)).to(torch.int32)
    u_dev, v_dev = u.to(dev), v.to(dev)
    vv, uu = torch.meshgrid(v.long(), u.long(), indexing="ij")
    vv, uu = vv.reshape(-1), uu.reshape(-1)
    npts = uv_size * uv_size
    xyz_dev, valid_dev, rgb_all = [], [], []
    # frames travel through two reusable pinned buffers (a copy from the loader's freshly allocated pageable batch costs
    # milliseconds on ROCm: the pages are pinned for the one transfer), results stay on the device until the end: one sync
    pinned, events, k = {}, [None, None], 0
    stream = torch.cuda.current_stream(dev)
    for rgb_imgs, depth_imgs, poses, K, _ in loader:
        bsz = len(rgb_imgs)
        if events[k] is not None:
            events[k].synchronize()
        staged = []
        for i, t in enumerate((depth_imgs.to(torch.float32), poses.to(torch.float32), K.to(torch.float32).inverse())):
            buf = pinned.get((k, i))
            if buf is None or buf.shape != t.shape:
                buf = pinned[(k, i)] = torch.empty(t.shape, dtype=torch.float32).pin_memory()
            buf.copy_(t)
            staged.append(buf.to(dev, non_blocking=True))
        ev = torch.cuda.Event()
        ev.record(stream)
        events[k], k = ev, 1 - k
        depth_d, poses_d, kinv_d = staged
        xyz = torch.empty((bsz, npts, 3), dtype=torch.float32, device=dev)
        valid = torch.empty((bsz, npts), dtype=torch.uint8, device=dev)
        for i in range(bsz):
            rc = lib().saf_backproject_lattice(
                depth_d[i].data_ptr(), dataset.imheight, dataset.imwidth, poses_d[i].data_ptr(), kinv_d[i].data_ptr(),
                u_dev.data_ptr(), uv_size, v_dev.data_ptr(), uv_size, float(max_depth), xyz[i].data_ptr(),
                valid[i].data_ptr(), stream.cuda_stream,
            )
            check(rc, "saf_backproject_lattice")
        for t in staged:
            t.record_stream(stream)
        xyz_dev.append(xyz)
        valid_dev.append(valid)
        rgb_all.append(rgb_imgs[:, vv, uu])
    if not xyz_dev:
        return torch.zeros((0, 3)), torch.zeros((0, 3))
    valid = torch.cat(valid_dev).bool().cpu()
    return torch.cat(xyz_dev).cpu()[valid], torch.cat(rgb_all)[valid]


def scene_bounds(xyz, voxel_size, trunc_m):
    """origin / nvox of the volume from the sparse cloud: 1st / 99th percentile -/+ trunc
    (reference clipfusion.py:1098-1106, clip_seem_fusion.py:278-287)."""
    pts = xyz.cpu().numpy() if isinstance(xyz, torch.Tensor) else np.asarray(xyz)
    minbound = torch.tensor(np.percentile(pts, 1, axis=0)).float() - trunc_m
    maxbound = torch.tensor(np.percentile(pts, 99, axis=0)).float() + trunc_m
    nvox = ((maxbound - minbound) / voxel_size).round().int()
    return minbound, nvox
