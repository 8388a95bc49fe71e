#!/usr/bin/env python3
"""Writes tests/golden/queue_trace.json: the library calls the queue behind integrate() makes, in order, over a list of
scenarios (SCENARIOS below) -- the schedule itself.  The device paths are bit-identical by design, so no comparison of volumes
notices a flush that takes another route (one saf_fuse_frames call where the session should be pushed); this trace does.
tests/test_queue_trace.py replays the scenarios and asserts the trace, token for token.  The host decisions depend on counts
and shapes alone (no event query, no synchronise feeds them), so the trace is deterministic.

The recorder sees two things only: the library boundary (a proxy around the loaded library object, on the cached handle of
spatially_aware_ai_amd._lib) and the modules' public surface (constructors, integrate, integrate_features, flush, reset, .cuda(),
buffer reads, state_dict, stats, borrow_inputs, the environment).  No internal name of the queue appears here: the file records
on one version of the host code and replays on another.

Token format, one string per call (every entry of the library that is not listed passes through unrecorded):

    stage*<count>@<first>-<last> <s> <rc>[ b]      <count> consecutive saf_stage_frame calls into ring slots first..last (slots
                                                  count modulo the ring: 511 is followed by 0); b: the descriptors carry no
                                                  images (borrow_inputs: depth / rgb / labels stay where the caller has them)
    create                                        saf_fuse_session_create (returned a handle; "create 0": it did not)
    ok <frames> -> <answer>                       saf_fuse_session_ok
    path <frames> -> <answer>                     saf_fuse_path
    prepare <frames> <s> <rc>                     saf_fuse_session_prepare (stream)
    push <frames> <s><s> ev<0|1> <rc>             saf_fuse_session_push (the queue's stream, the caller's stream; ev1: an event
                                                  was passed)
    finish <s> <rc> / abandon <s> <rc> / destroy  the session's other entries
    fuse <frames> <s> <rc>                        saf_fuse_frames
    recycled <frames> <s> <rc>                    saf_fuse_frames_recycled
    clear <s> <rc>                                saf_clear_unwritten_rows

<frames> = "<n>@<slot>:<img>": n frame descriptors; slot: the ring slot of the first one, from its `pose` address (poses are
always copied into the ring, 64 bytes per slot), or "-" when the pose lies in a tensor of the caller's (a direct call); img: "r"
when every frame's depth and rgb point into the ring (more exactly: not into a tensor the scenario handed in), "c" when they
point at the caller's tensors, "m" when the frames differ.  <s>: "c" when the stream argument is the current stream of the
module's device, "o" for another one.  A ring is recognised by its first use: a pose address that is neither the caller's nor
inside the ring known so far starts a new ring at slot 0 (a new ring is empty, so its first call is about slot 0).

Usage:  python tools/gen_queue_trace.py [--out tests/golden/queue_trace.json] [--only NAME ...]
(needs the MI355X; SAF_LIB_PATH selects the build to record from.)
"""
import argparse
import gc
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from spatially_aware_ai_amd import _abi, _lib  # noqa: E402
from spatially_aware_ai_amd import synthetic as syn  # noqa: E402

RING_SLOTS = 4 * _abi.SAF_WINDOW_FRAMES
POSE_BYTES = 64
RECORDED = ("saf_stage_frame", "saf_fuse_session_create", "saf_fuse_session_ok", "saf_fuse_session_prepare",
            "saf_fuse_session_push", "saf_fuse_session_finish", "saf_fuse_session_abandon", "saf_fuse_session_destroy",
            "saf_fuse_path", "saf_fuse_frames", "saf_fuse_frames_recycled", "saf_clear_unwritten_rows")


class Recorder:
    """Stands in for the loaded library: the RECORDED entries leave a token in ``tokens``, everything else is the library's."""

    def __init__(self, real):
        self._real = real
        self.tokens = []
        self.caller = []  # [lo, hi) address ranges of the tensors the scenario hands to the module
        self._lent = []   # ... and the tensors, alive while the recorder is: a freed range could become part of a ring
        self.ring = None  # address of the current ring's pose slot 0
        self._run = None  # the open run of saf_stage_frame calls: [count, first, last, tail]
        self._dev = torch.cuda.current_device()
        for name in RECORDED:
            setattr(self, name, self._wrap(name, getattr(real, name)))

    def __getattr__(self, name):  # (only what __init__ did not set: the unrecorded entries)
        return getattr(self._real, name)

    def lend(self, *tensors):
        self._lent.extend(tensors)
        for t in tensors:
            self.caller.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()))
        return tensors

    def _is_callers(self, addr):
        return any(lo <= addr < hi for lo, hi in self.caller)

    def _stream(self, s):
        return "c" if int(s or 0) == int(torch._C._cuda_getCurrentRawStream(self._dev)) else "o"

    def _slot(self, pose):
        pose = int(pose or 0)
        if self._is_callers(pose):
            return "-"
        off = None if self.ring is None else pose - self.ring
        if off is None or not (0 <= off < RING_SLOTS * POSE_BYTES and off % POSE_BYTES == 0):
            self.ring, off = pose, 0
        return off // POSE_BYTES

    def _frames(self, arr, n):
        kinds = {("c" if self._is_callers(int(arr[i].depth or 0)) else "r") + ("c" if self._is_callers(int(arr[i].rgb or 0)) else "r")
                 for i in range(n)}
        img = {frozenset(("rr",)): "r", frozenset(("cc",)): "c"}.get(frozenset(kinds), "m")
        return f"{n}@{self._slot(arr[0].pose)}:{img}"

    def _close_run(self):
        if self._run is not None:
            count, first, last, tail = self._run
            self.tokens.append(f"stage*{count}@{first}-{last} {tail}")
            self._run = None

    def _wrap(self, name, fn):
        def call(*a):
            rc = fn(*a)
            if name == "saf_stage_frame":
                dst = a[5]._obj
                slot = self._slot(dst.pose)
                tail = f"{self._stream(a[6])} {rc}" + (" b" if not dst.depth else "")
                run = self._run
                if run is not None and run[3] == tail and slot == (run[2] + 1) % RING_SLOTS:
                    run[0], run[2] = run[0] + 1, slot
                else:
                    self._close_run()
                    self._run = [1, slot, slot, tail]
                return rc
            self._close_run()
            short = name[len("saf_fuse_session_"):] if name.startswith("saf_fuse_session_") else name
            if short == "create":
                tok = "create" if rc else "create 0"
            elif short == "destroy":
                tok = "destroy"
            elif short in ("ok", "saf_fuse_path"):
                tok = f"{'ok' if short == 'ok' else 'path'} {self._frames(a[1], a[2])} -> {rc}"
            elif short == "prepare":
                tok = f"prepare {self._frames(a[2], a[3])} {self._stream(a[6])} {rc}"
            elif short == "push":
                tok = f"push {self._frames(a[2], a[3])} {self._stream(a[7])}{self._stream(a[9])} ev{int(bool(a[8]))} {rc}"
            elif short in ("finish", "abandon"):
                tok = f"{short} {self._stream(a[1])} {rc}"
            elif short == "saf_fuse_frames":
                tok = f"fuse {self._frames(a[1], a[2])} {self._stream(a[6])} {rc}"
            elif short == "saf_fuse_frames_recycled":
                tok = f"recycled {self._frames(a[1], a[2])} {self._stream(a[7])} {rc}"
            else:
                tok = f"clear {self._stream(a[3])} {rc}"
            self.tokens.append(tok)
            return rc

        return call


# ---- the scenarios ---------------------------------------------------------------------------------------------------------
GRID, W, H = (33, 30, 41), 64, 48  # the smallest shapes at which the queue still takes sessions (tests/test_session_lifecycle.py)
N_DISTINCT = 48  # frames generated per shape; the calls cycle through them (the trace depends on counts and shapes alone)


def _grid():
    return syn.make_grid(GRID, side=2.56 * GRID[0] / max(GRID))


def _build(seem, fdt, dim, **kw):
    from spatially_aware_ai_amd import ClipFusion, ClipSeemFusion
    from test_gpu_parity import FakeClip, FakeSeg

    g = _grid()
    if seem:
        return ClipSeemFusion(g.origin, g.voxel_size, g.nvox, g.trunc, False, 10, 10, FakeClip(dim), FakeSeg(), keep_xyz_world=False,
                              feat_dtype=fdt, **kw).cuda()
    return ClipFusion(g.origin, g.voxel_size, g.nvox, g.trunc, False, FakeClip(dim), None, 10, 10, keep_xyz_world=False, feat_dtype=fdt,
                      **kw).cuda()


def _frames(rec, seed, dim, seem=False, w=W, h=H, per_call=1, dtype=None):
    """Argument tuples for integrate_features, ``per_call`` frames each, on the device and known to the recorder."""
    npy, npx = syn.feature_map_shape(w, h)
    fr = syn.make_frames(seed, N_DISTINCT, width=w, height=h, feat_dim=dim, npy=npy, npx=npx, depth_kind="B")
    calls = []
    for i in range(0, N_DISTINCT - per_call + 1, per_call):
        part = fr[i:i + per_call]
        args = [torch.cat([f[k] for f in part]).cuda() for k in ("depth", "rgb", "pose", "K", "feat")]
        if dtype is not None:
            args = [t.to(dtype) for t in args]
        labs = [f["labels"].float().cuda() for f in part] if seem else None
        rec.lend(*args, *(labs or ()))
        calls.append(tuple(args) + (labs,))
    return calls


def _feed(mod, calls, n, start=0):
    for i in range(start, start + n):
        mod.integrate_features(*calls[i % len(calls)])


def s01_700_calls(rec):
    """The first window pushed chunk by chunk, later pushes one chunk behind, the ring wraps."""
    mod = _build(False, torch.float32, 256)
    _feed(mod, _frames(rec, 9101, 256), 700)
    mod.flush()
    return mod


def s02_five_frame_calls_and_a_reader(rec):
    """Chunk and window boundaries fall inside calls; a reader finishes the session mid-scan."""
    mod = _build(False, torch.float32, 256)
    calls = _frames(rec, 9102, 256, per_call=5)
    _feed(mod, calls, 40)
    mod.weight
    _feed(mod, calls, 10, start=40)
    mod.flush()
    return mod


def s03_borrowed_inputs(rec):
    mod = _build(False, torch.float32, 256)
    mod.borrow_inputs = True
    _feed(mod, _frames(rec, 9103, 256), 200)
    mod.flush()
    return mod


def s04_clipseem_bf16_labels(rec):
    mod = _build(True, torch.bfloat16, 512)
    _feed(mod, _frames(rec, 9104, 512, seem=True), 160)
    return mod


def s05_deferred_backbone(rec):
    """ClipFusion.integrate with this package's Clip: the backbone runs at the flush (the smallest configuration of
    test_backbone_deferred_to_the_flush_is_invisible)."""
    from spatially_aware_ai_amd import ClipFusion
    from spatially_aware_ai_amd.clipfusion import Clip
    from test_gpu_parity import _TileStatsBackbone

    g = syn.make_grid((32, 32, 64), side=2.56)
    clip = Clip("stub", None, backbone=_TileStatsBackbone(), tokenizer=None)
    mod = ClipFusion(g.origin, g.voxel_size, g.nvox, g.trunc, False, clip, None, 32, 32, keep_xyz_world=False).cuda()
    fr = syn.make_frames(9105, N_DISTINCT, width=96, height=64, feat_dim=8, npy=2, npx=3, depth_kind="B")
    calls = [rec.lend(*(f[k].cuda() for k in ("depth", "rgb", "pose", "K"))) for f in fr]
    for i in range(100):
        mod.integrate(*calls[i % len(calls)])
    return mod


def s06_reset_and_state_dict(rec):
    """Abandon, and the recycled call behind a lazy reset."""
    mod = _build(False, torch.float32, 256)
    calls = _frames(rec, 9106, 256)
    _feed(mod, calls, 100)
    mod.reset()
    _feed(mod, calls, 50)
    mod.state_dict()
    return mod


def s07_move_mid_scan(rec):
    """Destroy, and a new session."""
    mod = _build(False, torch.float32, 256)
    calls = _frames(rec, 9107, 256)
    _feed(mod, calls, 100)
    mod = mod.cuda()
    _feed(mod, calls, 100)
    mod.flush()
    return mod


def s08_shape_change(rec):
    """A key change makes a new ring."""
    mod = _build(False, torch.float32, 256)
    _feed(mod, _frames(rec, 9108, 256), 100)
    _feed(mod, _frames(rec, 9109, 256, w=32, h=24), 40)
    return mod


def s09_64_frame_windows(rec):
    """SAF_WIN_FRAMES=64: no session, the flushes go through saf_fuse_frames."""
    mod = _build(False, torch.float32, 256)
    _feed(mod, _frames(rec, 9110, 256), 200)
    return mod


def s10_fp16_inputs(rec):
    """The PyTorch-copy staging path: no saf_stage_frame call."""
    mod = _build(False, torch.float32, 256)
    _feed(mod, _frames(rec, 9111, 256, dtype=torch.float16), 70)
    return mod


def s11_direct_calls(rec):
    mod = _build(False, torch.float32, 256, defer_frames=False)
    mod.integrate_features(*_frames(rec, 9112, 256, per_call=16)[0])
    mod.integrate_features(*_frames(rec, 9113, 256, per_call=3)[0])
    return mod


def s12_few_frames_behind_a_reset(rec):
    """Five frames behind a lazy reset with no window open: the per-frame pipeline reads the rows it updates, so the flush is the
    recycled call."""
    mod = _build(False, torch.float32, 256)
    calls = _frames(rec, 9114, 256)
    _feed(mod, calls, 20)
    mod.reset()
    _feed(mod, calls, 5)
    mod.flush()
    return mod


SCENARIOS = {f.__name__: f for f in (s01_700_calls, s02_five_frame_calls_and_a_reader, s03_borrowed_inputs, s04_clipseem_bf16_labels,
                                     s05_deferred_backbone, s06_reset_and_state_dict, s07_move_mid_scan, s08_shape_change,
                                     s09_64_frame_windows, s10_fp16_inputs, s11_direct_calls,
                                     s12_few_frames_behind_a_reset)}
ENV = {"s09_64_frame_windows": {"SAF_WIN_FRAMES": "64"}}


def record(name):
    """Run one scenario under the recorder: {"trace": tokens, "pending": pending_frames at its end, "frames": stats()["frames"]}.
    The end state is read inside the recording (stats() flushes what is pending) and the module is dropped there too."""
    real = _lib.lib()
    env = ENV.get(name, {})
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    rec = Recorder(real)
    _lib._lib = rec
    try:
        mod = SCENARIOS[name](rec)
        pending = int(mod.pending_frames)
        frames = int(mod.stats()["frames"])
        del mod
        gc.collect()
        torch.cuda.synchronize()
        rec._close_run()
    finally:
        _lib._lib = real
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return {"trace": rec.tokens, "pending": pending, "frames": frames}


def write(path, scenarios):
    with open(path, "w") as f:
        f.write('{"ring_slots": %d, "scenarios": {\n' % RING_SLOTS)
        for si, (name, s) in enumerate(scenarios.items()):
            lines = ",\n".join("   " + json.dumps(s["trace"][i:i + 6])[1:-1] for i in range(0, len(s["trace"]), 6))
            f.write(' %s: {"pending": %d, "frames": %d, "trace": [\n%s\n  ]}%s\n'
                    % (json.dumps(name), s["pending"], s["frames"], lines, "," if si + 1 < len(scenarios) else ""))
        f.write("}}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "queue_trace.json"))
    ap.add_argument("--only", nargs="*", default=None)
    args = ap.parse_args()
    out = {name: record(name) for name in (args.only or SCENARIOS)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    write(args.out, out)
    print(args.out, {name: len(s["trace"]) for name, s in out.items()})


if __name__ == "__main__":
    main()
