#!/usr/bin/env python3
"""Writes tests/golden/row_kind_table.json: which (feat_dtype, accum_mode, direction) the fusion entries take and how they refuse
the others -- the legality matrix of the row kernels' kinds (RowKind, csrc/saf_fuse_dev.h), recorded from the build BEFORE the
kinds existed.  tests/test_row_kind_host.py replays it against the built library.

Every triple of {SAF_F32, SAF_BF16, SAF_F16} x {SAF_RUNNING_MEAN, SAF_SUM} x {forward, backward, backward_windowed} on an 8 x 8 x 8
volume of 512 channels (the narrowest width every dtype's windowed row kernel takes) with 16 frames of one shape (the fewest the
windowed path takes) and a workspace sized by saf_fuse_workspace_bytes_for_frames.  Nothing here makes a HIP call or follows a
pointer: the path queries never do, and each entry is asked in the way that ends before its first device call --

    forward            saf_fuse_path, saf_fuse_session_ok; saf_fuse_frames with no frames (SAF_OK behind the volume's checks)
    backward           saf_unfuse_path; saf_unfuse_frames with no frames (SAF_OK behind the volume's and the dtype / mode checks)
    backward_windowed  saf_unfuse_path; saf_unfuse_frames_windowed with the 16 frames and a MISALIGNED workspace pointer: a call
                       the entry takes ends at "workspace must be 256-byte aligned", the check behind the last refusal of a
                       combination; every other call ends at that refusal.

A record: dtype, accum, direction; "path" / "session": the queries' answers (-1: the volume itself is refused); "code": the
entry's return value; "error": saf_last_error() of a refusing entry (null otherwise); "phrase": the part of it that names the
reason (PHRASES; null otherwise).

Usage:  python tools/gen_row_kind_table.py [--out tests/golden/row_kind_table.json]     (SAF_LIB_PATH selects the build)
"""
import argparse
import ctypes as C
import itertools
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from spatially_aware_ai_amd import _abi  # noqa: E402

DTYPES = {"F32": _abi.SAF_F32, "BF16": _abi.SAF_BF16, "F16": _abi.SAF_F16}
ACCUMS = {"MEAN": _abi.SAF_RUNNING_MEAN, "SUM": _abi.SAF_SUM}
DIRECTIONS = ["forward", "backward", "backward_windowed"]
GRID, FEAT_DIM, N_FRAMES, H, W, NPY, NPX = (8, 8, 8), 512, 16, 480, 640, 30, 40
ADDR = 0x7F0000000000  # a non-null, 256-byte aligned placeholder: nothing follows it
# the reasons a combination is refused for, as the messages name them
PHRASES = ["SAF_SUM into an fp16 volume", "saf_unfuse_frames takes SAF_F32 volumes only", "saf_unfuse_frames takes SAF_RUNNING_MEAN volumes only",
           "saf_unfuse_frames_windowed takes SAF_F32 volumes only", "saf_unfuse_frames_windowed takes SAF_RUNNING_MEAN volumes only"]
ALIGNED = "workspace must be 256-byte aligned"  # no refusal of a combination: where an accepted backward_windowed call ends here


def triples():
    return itertools.product(DTYPES, ACCUMS, DIRECTIONS)


def evaluate(lib, dtype, accum, direction):
    v = _abi.SafVolume()
    v.nx, v.ny, v.nz = GRID
    v.feat_dim, v.n_classes, v.trunc = FEAT_DIM, 0, 0.1
    v.feat_dtype, v.accum_mode = DTYPES[dtype], ACCUMS[accum]
    for name in ("axis_x", "axis_y", "axis_z", "tsdf", "tsdf_weight", "weight", "rgb", "clip_feat"):
        setattr(v, name, ADDR)
    frames = (_abi.SafFrame * N_FRAMES)()
    for f in frames:
        f.height, f.width, f.npy, f.npx = H, W, NPY, NPX
        f.depth = f.rgb = f.pose = f.K = f.feat_map = ADDR
    ws = int(lib.saf_fuse_workspace_bytes_for_frames(C.byref(v), NPY, NPX, H, W))
    rec = {"dtype": dtype, "accum": accum, "direction": direction, "session": None}
    if direction == "forward":
        rec["path"] = lib.saf_fuse_path(C.byref(v), frames, N_FRAMES, ws)
        rec["session"] = lib.saf_fuse_session_ok(C.byref(v), frames, N_FRAMES, ws)
        rec["code"] = lib.saf_fuse_frames(C.byref(v), frames, 0, ADDR, ws, None, None)
    else:
        rec["path"] = lib.saf_unfuse_path(C.byref(v), frames, N_FRAMES, ws)
        if direction == "backward":
            rec["code"] = lib.saf_unfuse_frames(C.byref(v), frames, 0, ADDR, ws, None, None)
        else:
            rec["code"] = lib.saf_unfuse_frames_windowed(C.byref(v), frames, N_FRAMES, ADDR + 1, ws, None, None)
    rec["error"] = lib.saf_last_error().decode() if rec["code"] else None
    rec["phrase"] = next((p for p in PHRASES if rec["error"] and p in rec["error"]), None)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "row_kind_table.json"))
    args = ap.parse_args()
    from spatially_aware_ai_amd import _lib

    lib = _lib.lib()
    recs = [evaluate(lib, *t) for t in triples()]
    for r in recs:
        assert r["code"] == 0 or r["phrase"] or ALIGNED in r["error"], r
    with open(args.out, "w") as f:
        f.write("[\n" + ",\n".join(" " + json.dumps(r) for r in recs) + "\n]\n")
    print(args.out, len(recs), "records,", sum(r["phrase"] is not None for r in recs), "refusals of a combination")


if __name__ == "__main__":
    main()
