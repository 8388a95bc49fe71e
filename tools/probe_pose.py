"""Time refine_pose() at the benchmark's image size: a 640 x 480 depth image against a 256^3 volume fused from the coherent
analytic scene (the scene of tools/probe_raycast.py), from a look-at and a rolled pose moved by about a voxel.  The depth image
is what the volume shows of itself from the true pose.  Two timings per pose: the default levels and tolerances (the loop stops
when it has converged), and tolerances of 0 (all 14 iterations of the three levels run).  Median of 20 runs after warm-up, each
run timed by a pair of device events; one JSON line on stdout (times in ms).  Needs the MI355X: there is no fallback.

    python tools/probe_pose.py [--grid 256] [--frames 16] [--runs 20]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from probe_raycast import _Clip, _median_ms  # noqa: E402
from spatially_aware_ai_amd import ClipFusion  # noqa: E402
from spatially_aware_ai_amd import synthetic as syn  # noqa: E402


def _moved(pose, voxel):
    """``pose`` shifted by a voxel along (1, -1, 1) / sqrt(3) and turned by 4 mrad about the world's z."""
    c, s = torch.cos(torch.tensor(4e-3)), torch.sin(torch.tensor(4e-3))
    rot = torch.eye(4)
    rot[0, 0], rot[0, 1], rot[1, 0], rot[1, 1] = c, -s, s, c
    out = rot @ pose
    out[:3, 3] = pose[:3, 3] + voxel * torch.tensor([1.0, -1.0, 1.0]) / 3.0 ** 0.5
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--dim", type=int, default=32)  # (the refinement reads the TSDF alone)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--runs", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_pose needs the MI355X")
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
    res = {"probe": "pose", "grid": args.grid, "feat_dim": d, "pixels": [w, h], "frames": args.frames, "runs": args.runs,
           "unit": "ms, median / min / max of device-event times", "device": torch.cuda.get_device_name(0)}
    for name, pose in poses.items():
        depth = fz.render(pose.cuda(), k, h, w, rgb=False).depth
        start = _moved(pose, float(grid.voxel_size)).cuda()
        out = fz.refine_pose(depth, start, k)
        steps = int((out.log[:, 0] > 0).sum())
        res[name] = {"status": int(out.status), "steps": steps, "n_valid": int(out.n_valid),
                     "refine": _median_ms(lambda: fz.refine_pose(depth, start, k), args.runs),
                     "refine_all_14_steps": _median_ms(lambda: fz.refine_pose(depth, start, k, tol_t=0.0, tol_r=0.0), args.runs)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
