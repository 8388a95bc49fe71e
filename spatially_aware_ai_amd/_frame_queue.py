"""The deferred window queue behind ``integrate()``: its state, in one object, and the transitions that keep it consistent.

The reference calls integrate() with ONE frame per DataLoader batch (clip_seem_fusion.py:303-313, clipfusion.py:1120-1133).
One frame per C call would run the per-frame pipeline; the windowed path (saf_fuse_frames with 16+ frames: every touched feature
row travels to HBM once per 128-frame window) needs many frames in one call.  Small calls are therefore queued -- their inputs
copied into a staging ring of four windows (512 slots) -- and handed to the library 32 at a time (round 6): every 32 staged
frames are pushed into a streaming session (saf_fuse_session_push) on a stream of the queue's own -- one classification launch,
which runs beside the row kernel of the window before; the 128th frame of a window brings its row kernel -- and the caller's
stream goes on staging the next frames into the ring's other quarters meanwhile (rounds 2-5: one saf_fuse_frames call per flush
on the caller's stream -- every flush exposed its first window's classification, 3.7 ms, could not start before the window's
last frame was staged, 3 ms, and later frames' staging kernels queued behind the flush, 3 ms: 0.86-0.90 of the bulk rate).
Whatever reads or replaces the volume -- the registered buffers (attribute access, state_dict, .to()), stats(), extract_mesh,
the merge -- pushes what is staged, finishes the session and lets its stream wait for it.  The device paths are bit-identical,
so a caller cannot tell -- except by speed.

Who owns what.  ``FrameQueue`` (one per fusion module, in the module's ``__dict__`` as ``_queue``): the pending count, the ring,
the session handle and whether a window's row kernel is owed, the queue's stream with its last event and the allocations marked
for it, and the launch flag of the flush in progress.  ``StagingRing`` (one per frame shape, ``FrameQueue.ring``): the staging
tensors, the reusable descriptors, what was borrowed, and the ring's progress with its events.  Neither holds a reference to the
module (a module whose last reference goes away is freed at once, its session destroyed by ``__del__``): the functions that need
the module's buffers, workspace or descriptors take it as an argument.  The mixin keeps the decisions (`_fuse`: queue or fuse
now; `_flush_pending`: what a flush hands over and what a failure leaves; `_fuse_now`: session or one call).

Transitions, each defined here once: ``StagingRing.all_free_behind`` (every quarter free behind an event, the session starts
over), ``StagingRing.release_borrowed`` (a slot's, or all, borrowed inputs), ``FrameQueue.abandon`` (reset(): the open window is
dropped with the volume), ``FrameQueue.close`` (no session, no stream, no ring: a move, the module's end).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _abi
from ._lib import SafError, check, lib

_WIN = _abi.SAF_WINDOW_FRAMES


class StagingRing:
    """The staging ring of one frame shape.  ``key``: (h, w, feature map shape, labels?, rgb_bilinear, deferred backbone or None)
    -- frames queued together share the shapes and, for deferred features, the backbone call and its autocast state."""

    __slots__ = ("key", "depth", "rgb", "pose", "K", "feat", "labels", "base", "step", "src", "dst", "lazy", "bptr", "brefs",
                 "ring0", "free_ev", "sess_frames", "chunk_ready", "ready_evs")

    def __init__(self, key, lazy, n_slots, dev):
        h, w, fshape, has_labels = key[:4]
        mk = lambda *shape: torch.empty((n_slots,) + shape, dtype=torch.float32, device=dev)
        self.key = key
        self.depth, self.rgb, self.pose, self.K = mk(h, w), mk(h, w, 3), mk(4, 4), mk(3, 3)
        self.feat = mk(*fshape)
        self.labels = mk(h, w) if has_labels else None
        # base addresses and byte strides of the ring's slots (no tensor views per call)
        self.base = tuple(t.data_ptr() if t is not None else 0 for t in (self.depth, self.rgb, self.pose, self.K, self.feat, self.labels))
        self.step = (4 * h * w, 12 * h * w, 64, 36, 4 * fshape[0] * fshape[1] * fshape[2], 4 * h * w)
        # the two descriptors saf_stage_frame is called with, refilled per frame
        self.src = _abi.SafFrame(h, w, None, None, None, None, None, fshape[1], fshape[2], None, 0)
        self.dst = _abi.SafFrame(h, w, None, None, None, None, None, fshape[1], fshape[2], None, 0)
        self.lazy = lazy  # (fn, autocast enabled, autocast dtype) of a deferred backbone, or None
        # borrow_inputs: per slot the addresses of the caller's depth / rgb / label images that were NOT copied (0: the ring's)
        # and the tensors themselves, held until the slot is staged again (behind its row kernel's event)
        self.bptr = np.zeros((n_slots, 3), dtype=np.int64)
        self.brefs = [None] * n_slots
        # the frames staged and not yet handed over lie in slots [ring0, ring0 + pending); free_ev[q]: the event behind the row
        # kernel that reads quarter q's frames (None: free)
        self.ring0 = 0
        self.free_ev = [None] * (n_slots // _WIN)
        self.sess_frames = 0   # frames the session has taken since it started over: its windows are the ring's quarters
        self.chunk_ready = {}  # slot behind a prepared chunk -> the event behind its staging and depth tiles
        self.ready_evs = []    # the last eight events given to a push (kept alive while the device may still wait for them)

    def all_free_behind(self, ev):
        """Every quarter's frames are free behind ``ev``, and the session starts over (at its next push)."""
        self.free_ev = [ev] * len(self.free_ev)
        self.sess_frames = 0
        self.chunk_ready = {}

    def release_borrowed(self, slot=None):
        """Forget the borrowed tensors of ``slot``, or of every slot."""
        if slot is None:
            if any(r is not None for r in self.brefs):
                self.brefs = [None] * len(self.brefs)
                self.bptr[:] = 0
        elif self.brefs[slot] is not None:
            self.bptr[slot] = 0
            self.brefs[slot] = None


class FrameQueue:
    """The queue of one fusion module."""

    __slots__ = ("pending", "ring", "session", "session_open", "stream", "event", "seen", "launched")

    def __init__(self):
        self.pending = 0           # frames staged and not yet handed to the library
        self.ring = None           # the StagingRing of the current frame shape
        self.session = None        # saf_fuse_session handle of the queue's flushes (created at the first one)
        self.session_open = False  # a pushed window's row kernel is still owed (saf_fuse_session_finish)
        self.stream = None         # the queue's own stream: a flush runs beside the staging of later frames
        self.event = None          # recorded behind the last push / finish: whoever reads the volume waits for it
        self.seen = set()          # data_ptr of the allocations already marked for `stream` (record_stream); only grows until close()
        self.launched = False      # the flush in progress has launched kernels (a failure after that poisons the volume)

    def busy(self):
        """Frames staged but not handed over, or a pushed window whose row kernel is still owed."""
        return bool(self.pending or self.session_open)

    # -- transitions ---------------------------------------------------------------------------------------------------------
    def close(self):
        """No session, no stream, no ring: the session's classification stream and events, the queue's stream and the ring
        belong to the device the module leaves (a move; the caller has joined them), or the module is going away."""
        if self.session:
            lib().saf_fuse_session_destroy(self.session)
        self.session = None
        self.session_open = False
        self.ring = None
        self.stream = None
        self.event = None
        self.seen = set()

    def abandon(self, dev):
        """reset(): a pushed window whose row kernel is still owed is dropped with the volume; what the queue's stream and the
        library's classification stream already run must finish before the buffers are zeroed: the abandon lets the queue's
        stream wait for the classification stream, the event recorded behind that wait covers both, and the current stream waits
        for it.  Kept as found: without a queue stream (the flushes went through saf_fuse_frames, as under SAF_WIN_FRAMES=64) the
        ring keeps its `ring0` and its quarter events; borrowed tensors are not released here but when their slots are staged
        again or at the next final flush."""
        fs = self.stream
        if fs is None:
            return
        if self.session is not None:
            with torch.cuda.device(dev):
                check(lib().saf_fuse_session_abandon(self.session, fs.cuda_stream), "saf_fuse_session_abandon")
        self.session_open = False
        ev = fs.record_event()
        self.event = ev
        torch.cuda.current_stream(dev).wait_event(ev)
        if self.ring is not None:
            self.ring.ring0 = 0
            self.ring.all_free_behind(ev)

    # -- streams -------------------------------------------------------------------------------------------------------------
    def own_stream(self, dev, tensors):
        """The queue's own stream (created at the first push); ``tensors`` it is about to use are marked for the allocator
        (record_stream, once per allocation: whoever frees them -- a deleted module, a regrown workspace -- must not hand the
        memory out while that stream still reads it)."""
        fs = self.stream
        if fs is None:
            fs = self.stream = torch.cuda.Stream(device=dev)
        seen = self.seen
        for t in tensors:
            if t is not None and t.data_ptr() not in seen:
                seen.add(t.data_ptr())
                t.record_stream(fs)
        return fs

    def wait(self, module):
        """The current stream waits for what the queue's stream has been given (readers of the volume)."""
        ev = self.event
        if ev is not None:
            dev = module._buffers["tsdf"].device
            torch.cuda.current_stream(dev).wait_event(ev)

    def finish_session(self, module):
        """Launch the row kernel of the window the session still holds (on the queue's stream) and let the current stream wait."""
        if not self.session_open:
            self.wait(module)
            return
        dev = module._buffers["tsdf"].device
        fs = self.stream
        with torch.cuda.device(dev):
            rc = lib().saf_fuse_session_finish(self.session, fs.cuda_stream)
            self.session_open = False
            ev = fs.record_event()
            self.event = ev
            if self.ring is not None:  # the open window's frames (and, conservatively, everybody's) are free behind `ev`
                self.ring.all_free_behind(ev)
            if rc != 0:  # its windows are classified and partly fused: nothing to retry
                module.__dict__["_poisoned"] = "the queue's session could not launch its last row kernel; the volume is incomplete: reset() it"
            check(rc, "saf_fuse_session_finish")
            torch.cuda.current_stream(dev).wait_event(ev)

    # -- the session ---------------------------------------------------------------------------------------------------------
    def prepare_chunk(self, module, ring, lo, n, stream):
        """``saf_fuse_session_prepare`` for the staged frames in ring slots [lo, lo + n): their depth tiles, on ``stream`` behind
        their staging, and the event a later push looks at (``hipEventQuery``).  A shape no session takes: nothing to do."""
        if module.__dict__.get("_poisoned") or getattr(module, "_shard_stripes", None) is not None:
            return
        sl = slice(lo, lo + n)
        labs = None if ring.labels is None else ring.labels[sl]
        arr, _keep, npy, npx = module._make_frames(ring.depth[sl], ring.rgb[sl], ring.pose[sl], ring.K[sl], ring.feat[sl], labs, ring.key[4],
                                                   borrowed=ring.bptr[sl])
        vol = module._c_volume(for_fuse=True)
        ws = module._get_workspace(npy, npx, (int(ring.depth.shape[1]), int(ring.depth.shape[2])))
        L = lib()
        if L.saf_fuse_session_ok(C.byref(vol), arr, n, ws.numel()) != 1:
            return
        if self.session is None:
            self.session = L.saf_fuse_session_create()
        if L.saf_fuse_session_prepare(self.session, C.byref(vol), arr, n, ws.data_ptr(), ws.numel(), stream.cuda_stream) == 0:
            ring.chunk_ready[lo + n] = stream.record_event()  # keyed by the slot behind the chunk

    def push(self, module, vol, arr, ws, lo, n, dev, stream):
        """Push the staged frames ``arr`` (ring slots [lo, lo + n)) into the session on the queue's own stream; their last
        window's row kernel stays owed (``finish_session``).  ``stream``: the current stream of ``dev``, which staged them."""
        L = lib()
        ring = self.ring
        b = module._buffers
        fs = self.own_stream(dev, [ws, ring.depth, ring.rgb, ring.pose, ring.K, ring.feat, ring.labels] +
                             [b.get(k) for k in ("tsdf", "tsdf_weight", "weight", "rgb", "clip_feat", "labels_one_hot",
                                                 "axis_x", "axis_y", "axis_z", "fuse_stats")])
        # the staging kernels (and a deferred backbone's maps) of these frames: what their classification waits for -- NOT
        # the queue's stream, where the previous window's row kernel sits (the launches are to run beside it).  The
        # session's first push also orders the queue's stream behind the caller's (reset()'s zeroing, an earlier finish)
        # (a chunk whose tiles were prepared a chunk ago brings the event recorded behind them -- completed by now, the
        #  library finds, and waits for nothing; anything else: an event behind what this stream holds now)
        ready = ring.chunk_ready.pop(lo + n, None)
        if ready is None or ring.lazy is not None:  # (a deferred backbone has just written these frames' maps: behind THAT)
            ready = stream.record_event()
        for k in [k for k in ring.chunk_ready if k <= lo + n]:
            del ring.chunk_ready[k]
        if not self.session_open:
            fs.wait_event(ready)
        if self.session is None:
            self.session = L.saf_fuse_session_create()
        # (the depth tiles of these frames: on the caller's stream, behind their staging -- out of the classification chain)
        rc = L.saf_fuse_session_push(self.session, C.byref(vol), arr, len(arr), ws.data_ptr(), ws.numel(),
                                     b["fuse_stats"].data_ptr(), fs.cuda_stream, ready.cuda_event, stream.cuda_stream)
        ring.ready_evs.append(ready)  # (kept alive while the device may still wait for them)
        del ring.ready_evs[:-8]
        # SAF_E_INVALID / _WORKSPACE / _UNSUPPORTED come from the checks at the entry (every frame descriptor is validated
        # before the first launch); a HIP error may have left some windows fused (see _flush_pending)
        self.launched = rc == 0 or rc == _abi.SAF_E_HIP
        if rc == 0:
            self.session_open = True
            ev = fs.record_event()
            self.event = ev
            # the session's windows are the ring's quarters (a session starts at slot 0): the windows this push completed
            # have their row kernels queued -- behind `ev` their frames are free
            w0, w1 = ring.sess_frames // _WIN, (ring.sess_frames + n) // _WIN
            for w in range(w0, w1):
                ring.free_ev[w % len(ring.free_ev)] = ev
            ring.sess_frames += n
        check(rc, "saf_fuse_session_push")

    # -- staging -------------------------------------------------------------------------------------------------------------
    def stage(self, module, ring, depth_imgs, rgb_imgs, poses, K, clip_feat_img, label_maps, borrow_ok):
        """Copy a call's frames into the ring's next slots (``clip_feat_img`` None: a deferred backbone, nothing to copy for the
        maps) and hand over what is due: after every 32nd slot the chunk's depth tiles are prepared and a chunk is pushed.
        ``borrow_ok``: the module's ``borrow_inputs``."""
        f32 = torch.float32
        lazy = clip_feat_img is None
        bsz = int(depth_imgs.shape[0])
        n_ring, n_push = module._QUEUE_FRAMES, module._PUSH_FRAMES
        dev = module._buffers["tsdf"].device
        with torch.cuda.device(dev):
            # current_stream(dev), not current_stream(): without a device torch asks is_available() first, which looks up
            # an environment variable by raising and catching a KeyError -- up to 100 us per call in a long-lived process
            stream = torch.cuda.current_stream(dev)
            fast = lazy or (
                all(t.dtype == f32 for t in (depth_imgs, rgb_imgs, poses, K, clip_feat_img)) and depth_imgs.is_contiguous()
                and rgb_imgs.is_contiguous() and poses.is_contiguous() and K.is_contiguous() and
                (label_maps is None or all(m.dtype == f32 and m.is_contiguous() for m in label_maps)))
            src, dst, base, step = ring.src, ring.dst, ring.base, ring.step
            feat_dim = ring.key[2][0]
            # (a deferred backbone reads the queued frames' rgb from the ring: nothing to borrow there)
            borrow = fast and not lazy and borrow_ok
            raw_stream = stream.cuda_stream
            if fast:
                fs = (0, 0, 0, 0) if lazy else clip_feat_img.stride()
                sp = (depth_imgs.data_ptr(), rgb_imgs.data_ptr(), poses.data_ptr(), K.data_ptr(),
                      0 if lazy else clip_feat_img.data_ptr())
            for i in range(bsz):
                k = self.pending
                if ring.ring0 + k >= n_ring:
                    # a full ring means an earlier flush failed and kept its frames: try again (it re-raises) -- never
                    # stage into a slot beyond the ring
                    module._flush_pending()
                    k = self.pending
                    if ring.ring0 + k >= n_ring:
                        raise SafError("the staging ring is full and could not be flushed")
                slot = ring.ring0 + k
                if slot % _WIN == 0:  # a quarter of the ring is reused: the row kernel that read its frames must be done
                    ev = ring.free_ev[slot // _WIN]
                    if ev is not None:
                        stream.wait_event(ev)
                        ring.free_ev[slot // _WIN] = None
                if fast:  # one launch per frame (saf_stage_frame); addresses by arithmetic: no tensor views, no new descriptors
                    src.depth, src.rgb, src.pose = sp[0] + i * step[0], sp[1] + i * step[1], sp[2] + i * 64
                    src.K, src.feat_map = sp[3] + i * 36, (None if lazy else sp[4] + i * fs[0] * 4)
                    dst.depth, dst.rgb, dst.pose = base[0] + slot * step[0], base[1] + slot * step[1], base[2] + slot * step[2]
                    dst.K, dst.feat_map = base[3] + slot * step[3], base[4] + slot * step[4]
                    if label_maps is not None:
                        src.label_map, dst.label_map = label_maps[i].data_ptr(), base[5] + slot * step[5]
                    if borrow:  # the images stay where the caller has them: 5 MB per frame that are not copied
                        ring.bptr[slot] = (src.depth, src.rgb, src.label_map or 0)
                        ring.brefs[slot] = (depth_imgs, rgb_imgs, None if label_maps is None else label_maps[i])
                        src.depth = src.rgb = src.label_map = dst.depth = dst.rgb = dst.label_map = None
                    elif ring.brefs[slot] is not None:
                        ring.release_borrowed(slot)
                    check(lib().saf_stage_frame(C.byref(src), feat_dim, fs[1], fs[2], fs[3], C.byref(dst), raw_stream),
                          "saf_stage_frame")
                else:  # other dtypes / layouts: PyTorch copies convert
                    if ring.brefs[slot] is not None:
                        ring.release_borrowed(slot)
                    ring.depth[slot].copy_(depth_imgs[i], non_blocking=True)
                    ring.rgb[slot].copy_(rgb_imgs[i], non_blocking=True)
                    ring.pose[slot].copy_(poses[i], non_blocking=True)
                    ring.K[slot].copy_(K[i], non_blocking=True)
                    ring.feat[slot].copy_(clip_feat_img[i], non_blocking=True)
                    if label_maps is not None:
                        ring.labels[slot].copy_(label_maps[i], non_blocking=True)
                self.pending = k + 1
                if (slot + 1) % n_push == 0:
                    # one classification launch's worth of frames is staged: their depth tiles are computed now, behind the staging
                    # on this stream, and the chunk BEFORE them is handed over -- its staging and tiles have completed meanwhile
                    # (the host needs 0.7 ms to stage 32 frames), so its launch is queued with no cross-stream wait in front
                    # (a session's FIRST window is pushed chunk by chunk at once, each launch waiting for its frames: nothing runs
                    #  beside it yet, a barrier in front of a launch costs nothing there, and the scan starts 0.7 ms earlier)
                    self.prepare_chunk(module, ring, slot + 1 - n_push, n_push, stream)
                    if ring.sess_frames < _WIN:
                        module._flush_pending()
                    elif self.pending > n_push:
                        module._flush_pending(keep=n_push)
            if fast:  # the sources are read asynchronously on this stream
                for t in (depth_imgs, rgb_imgs, poses, K) + (() if lazy else (clip_feat_img,)) + tuple(label_maps or ()):
                    t.record_stream(stream)
