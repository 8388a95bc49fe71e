#!/usr/bin/env python3
"""Removal rate of the windowed removal (saf_unfuse_frames_windowed) against the per-frame removal (saf_unfuse_frames) on the same
frames, and the windowed forward path on them for the ratio (the figures under profiles/r15/ come from this script).

The setting of DESIGN 4.17's throughput paragraph: a 256^3 x 512 f32 volume, 640 x 480 frames, random depth from the benchmark's
generator.  Per frame count: the frames are fused (timed: the windowed forward path) and taken out again (timed), the two removals
alternated, `--repeats` times after one untimed pass of each; device events around each C call; the volume is empty again after
every pair, which the script checks at the end.  Needs the MI355X.

    python tools/measure_unfuse.py [--grid 256] [--dim 512] [--counts 16,32,64,128,256] [--repeats 3] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--counts", default="16,32,64,128,256")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    counts = [int(c) for c in a.counts.split(",")]

    import torch

    import bench
    from spatially_aware_ai_amd import ClipFusion
    from spatially_aware_ai_amd import synthetic as syn
    from spatially_aware_ai_amd._lib import check, lib

    assert torch.cuda.is_available(), "the measurement needs the MI355X"
    device = torch.device("cuda:0")
    npy, npx = syn.feature_map_shape(a.width, a.height)
    grid = syn.make_grid((a.grid,) * 3)

    class Resident:
        feature_dim = a.dim

    fz = ClipFusion(grid.origin, grid.voxel_size, grid.nvox, grid.trunc, False, Resident(), None, a.height // 3, a.height // 6,
                    keep_xyz_world=False, device=device).to(device)
    n_max = max(counts)
    depth, rgb, poses, ks, feat = bench.gen_frames_gpu(n_max, a.width, a.height, a.dim, npy, npx, "A", 1000, device)
    arr, keep, _, _ = fz._make_frames(depth, rgb, poses, ks, feat, None, False)
    ws = fz._get_workspace(npy, npx, (a.height, a.width))
    vol = fz._c_volume(for_fuse=True)
    stats = fz._buffers["fuse_stats"]
    L = lib()
    stream = torch.cuda.current_stream().cuda_stream

    def timed(entry, name, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(entry(C.byref(vol), arr, n, ws.data_ptr(), ws.numel(), stats.data_ptr(), stream), name)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    lines, rows = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# {a.grid}^3 x {a.dim} f32 running mean, {a.width} x {a.height} frames, random depth; ms per call, {a.repeats} repeats after one "
        "untimed pass; device events")
    say(f"# {'frames':>6s}  {'windowed removal':>26s}  {'per-frame removal':>26s}  {'windowed forward':>26s}  ratio pf/win (medians)")
    for n in counts:
        takes = L.saf_unfuse_path(C.byref(vol), arr, n, ws.numel())
        assert takes == 1 and L.saf_fuse_path(C.byref(vol), arr, n, ws.numel()) == 1, (n, takes)
        t = {"win": [], "pf": [], "fwd": []}
        for rep in range(a.repeats + 1):
            for which, entry, name in (("win", L.saf_unfuse_frames_windowed, "saf_unfuse_frames_windowed"),
                                       ("pf", L.saf_unfuse_frames, "saf_unfuse_frames")):
                f = timed(L.saf_fuse_frames, "saf_fuse_frames", n)
                r = timed(entry, name, n)
                if rep > 0:
                    t["fwd"].append(f)
                    t[which].append(r)
        med = lambda x: sorted(x)[len(x) // 2]
        fmt = lambda x: " / ".join(f"{v:.2f}" for v in x)
        say(f"  {n:6d}  {fmt(t['win']):>26s}  {fmt(t['pf']):>26s}  {fmt(t['fwd'][::2]):>26s}  {med(t['pf']) / med(t['win']):.2f}")
        rows.append({"frames": n, "windowed_removal_ms": t["win"], "per_frame_removal_ms": t["pf"], "windowed_forward_ms": t["fwd"],
                     "ms_per_frame": {k: med(v) / n for k, v in t.items()}})
    s = stats.cpu().tolist()
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    empty = not any(bool((bits(getattr(fz, name)) != 0).any()) for name in ("tsdf", "tsdf_weight", "weight", "rgb"))
    # (the feature volume in slices: a comparison over 34 GB at once would need another 8)
    feat_bits = bits(fz.clip_feat)
    step = max(1, feat_bits.shape[0] // 64)
    empty = empty and not any(bool((feat_bits[i:i + step] != 0).any()) for i in range(0, feat_bits.shape[0], step))
    say(f"# the volume is bit for bit empty again: {empty}; skipped {s[13]} / {s[14]}")
    say(json.dumps({"grid": a.grid, "dim": a.dim, "width": a.width, "height": a.height, "rows": rows, "empty_again": empty}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    assert empty and s[13] == 0 and s[14] == 0


if __name__ == "__main__":
    main()
