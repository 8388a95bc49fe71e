"""Time saf_object_stats at the benchmark's size: a 256^3 x 512 volume (f32, then bf16) fused from the coherent analytic scene
with its panoptic labels (label_kind="scene": every pixel carries the class of the surface it sees, as SyntheticScan's frames do),
objects from its own discover_objects result -- beside the route a caller had before the entry
existed: row normalisation plus index_add_ in torch on the same inputs.  Median of 20 runs after warm-up, each run timed by a
pair of device events; one JSON line on stdout (times in ms).  `frac` is the algorithmic traffic, 8 N + M (D s + 16) bytes for
M fused members of s-byte elements, over the kernel's time, as a share of the copy rate measured here (a 1 GiB device copy,
bytes read + written).  Needs the MI355X: there is no fallback.

    python tools/probe_objects.py [--grid 256] [--frames 16] [--runs 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spatially_aware_ai_amd import ClipSeemFusion, discover_objects  # noqa: E402
from spatially_aware_ai_amd import synthetic as syn  # noqa: E402
from spatially_aware_ai_amd.objects import object_slots, object_stats  # noqa: E402


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


def _copy_rate(runs):
    src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    ms = _median_ms(lambda: dst.copy_(src), runs)[0]
    return 2.0 * src.numel() / (ms * 1e-3) / 1e9


def _torch_route(weight, clip_feat, slot, k):
    """What a caller could do on the parent commit: gather the fused members' rows, normalise, index_add_."""
    sel = torch.nonzero((slot >= 0) & (weight > 0)).reshape(-1)
    f = clip_feat[sel].float()
    f = torch.nan_to_num(f / f.norm(dim=1, keepdim=True), nan=0.0)
    idx = slot[sel].long()
    out = torch.zeros((k, f.shape[1]), dtype=torch.float32, device=f.device).index_add_(0, idx, f)
    return out / torch.bincount(idx, minlength=k).clamp_min(1)[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--runs", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_objects needs the MI355X")
    w, h, d = 640, 480, args.dim
    npy, npx = syn.feature_map_shape(w, h)
    grid = syn.make_grid(args.grid)
    names = syn.scene_class_names()
    frames = syn.make_frames(778, args.frames, width=w, height=h, feat_dim=d, npy=npy, npx=npx, depth_kind="B", label_kind="scene")
    cat = lambda k: torch.cat([f[k] for f in frames]).cuda()
    res = {"probe": "object_stats", "grid": args.grid, "feat_dim": d, "frames": args.frames, "runs": args.runs,
           "unit": "ms, median / min / max of device-event times", "device": torch.cuda.get_device_name(0),
           "copy_GBps": round(_copy_rate(args.runs), 1)}
    for name, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        fz = ClipSeemFusion(grid.origin, grid.voxel_size, grid.nvox, grid.trunc, False, 10, 10, _Clip(d), None,
                            keep_xyz_world=False, feat_dtype=dtype, device="cuda").cuda()
        fz.integrate_features(cat("depth"), cat("rgb"), cat("pose"), cat("K"), cat("feat"), [f["labels"].float().cuda() for f in frames])
        fz.flush()
        nvox = tuple(int(v) for v in fz.nvox)
        know, voxel_obj_idx = discover_objects(fz.label_index().view(*nvox), names, arrays=True)
        slot, ids = object_slots(voxel_obj_idx, know)
        k, n = len(ids), slot.numel()
        weight, rgb, feat = fz.weight, fz.rgb, fz.clip_feat
        torch.cuda.synchronize()
        m = int(((slot >= 0) & (weight > 0)).sum())
        shell = int((weight > 0).sum())
        # the scene's surfaces are walls, floor, ceiling, window and a sphere: most of the fused shell belongs to some object
        assert k > 0, "discover_objects found no object: the labels are not the scene's"
        assert 2 * m >= shell > 0, f"only {m} of the {shell} fused voxels belong to an object: the row path would hardly be measured"
        algo = 8 * n + m * (d * feat.element_size() + 16)
        t_kernel = _median_ms(lambda: object_stats(weight, rgb, feat, nvox, slot, k), args.runs)
        t_torch = _median_ms(lambda: _torch_route(weight, feat, slot, k), args.runs)
        got = object_stats(weight, rgb, feat, nvox, slot, k)["feat"]
        gbps = algo / (t_kernel[0] * 1e-3) / 1e9
        res[name] = {"N": n, "K": k, "M": m, "fused_voxels": shell, "members": int((slot >= 0).sum()), "algorithmic_bytes": algo,
                     "saf_object_stats": t_kernel, "torch_normalise_index_add": t_torch, "achieved_GBps": round(gbps, 1),
                     "frac": round(gbps / res["copy_GBps"], 4),
                     "max_abs_diff_to_torch": float((got - _torch_route(weight, feat, slot, k)).abs().max())}
        del fz, weight, rgb, feat, got
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
