"""Time render() and render_query() at the benchmark's size: 640 x 480 pixels over a 256^3 x 512 fp32 volume fused from the
coherent analytic scene, from one look-at pose and one rolled pose.  Median of 20 runs after warm-up, each run timed by a pair
of device events; one JSON line on stdout (times in ms).  Needs the MI355X: there is no fallback.

    python tools/probe_raycast.py [--grid 256] [--frames 16] [--runs 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spatially_aware_ai_amd import ClipFusion  # noqa: E402
from spatially_aware_ai_amd import synthetic as syn  # noqa: E402


class _Clip:
    def __init__(self, d):
        self.feature_dim = d


def _median_ms(fn, runs, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--runs", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_raycast needs the MI355X")
    w, h, d = 640, 480, args.dim
    npy, npx = syn.feature_map_shape(w, h)
    grid = syn.make_grid(args.grid)
    fz = ClipFusion(grid.origin, grid.voxel_size, grid.nvox, grid.trunc, False, _Clip(d), None, 10, 10, keep_xyz_world=False).cuda()
    frames = syn.make_frames(778, args.frames, width=w, height=h, feat_dim=d, npy=npy, npx=npx, depth_kind="B")
    cat = lambda k: torch.cat([f[k] for f in frames]).cuda()
    fz.integrate_features(cat("depth"), cat("rgb"), cat("pose"), cat("K"), cat("feat"))
    fz.flush()
    torch.cuda.synchronize()
    gen = torch.Generator().manual_seed(3)
    centre = torch.tensor([1.2, -1.9, 1.1])
    poses = {"look_at": syn.look_at_pose(centre), "rolled": syn.family_pose(gen, centre, "roll")}
    k = syn.intrinsics(w, h).cuda()
    texts = {n: syn.class_embeddings(d, n_classes=n).cuda() for n in (5, 63)}
    res = {"probe": "raycast", "grid": args.grid, "feat_dim": d, "pixels": [w, h], "frames": args.frames, "runs": args.runs,
           "unit": "ms, median / min / max of device-event times", "device": torch.cuda.get_device_name(0)}
    for name, pose in poses.items():
        p = pose.cuda()
        out = fz.render(p, k, h, w)
        res[name] = {"hit_share": round(float(out.hit.float().mean()), 4),
                     "render": _median_ms(lambda: fz.render(p, k, h, w), args.runs),
                     "render_no_rgb": _median_ms(lambda: fz.render(p, k, h, w, rgb=False), args.runs)}
        for n, t in texts.items():
            res[name][f"render_query_L{n}"] = _median_ms(lambda: fz.render_query(t, p, k, h, w), args.runs)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
