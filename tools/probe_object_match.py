"""saf_object_overlap at the benchmark's grid: two 256^3 slot grids, offset 0 (the whole grid overlaps: 134 MB read at the least),
beside a torch restatement on the same tensors (mask, key = a (n_b + 1) + b, ``torch.bincount``, sums of the table's rows and columns).
  boxes         about 200 boxes per version filling about 10 % of the voxels; version b is version a with every box shifted by up
                to 2 voxels per axis, a tenth of the boxes dropped and as many new ones added
  checkerboard  two objects alternating voxel by voxel in all three directions, in both grids: runs of length 1
  noise         every voxel a member of one of 200 objects drawn at random, in both grids: some 500 distinct keys in a chunk of
                512 voxels, the case in which the pass does issue about one atomic per voxel
Device times by HIP events, REPEATS repetitions after a warm-up, the two candidates alternating; nothing else may run on the GPU.
Then ``extend_scene(keep_identities=True)`` on the scene of tests/test_scene_extend_gpu.py, for its ``identities`` lap beside the
other laps.  Usage: python tools/probe_object_match.py [out.json]   (profiles/r12/object_match.json is its output)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spatially_aware_ai_amd import synthetic as syn
from spatially_aware_ai_amd.objects import object_overlap

REPEATS = 5
NV = 256


def ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(v):
    s = sorted(v)
    return {"ms": [round(x, 3) for x in v], "median_ms": round(s[len(s) // 2], 3), "spread_ms": round(s[-1] - s[0], 3)}


def torch_overlap(a, b, n_a, n_b):
    ma, mb = (a >= 0) & (a < n_a), (b >= 0) & (b < n_b)
    key = torch.where(ma, a, n_a).long() * (n_b + 1) + torch.where(mb, b, n_b)
    table = torch.bincount(key, minlength=(n_a + 1) * (n_b + 1)).view(n_a + 1, n_b + 1)
    return {"pair": table[:n_a, :n_b].contiguous(), "in_a": table[:n_a].sum(1), "in_b": table[:, :n_b].sum(0)}


def boxes(rng, n_boxes):
    lo = np.stack([rng.integers(0, NV - 28, n_boxes) for _ in range(3)], axis=1)
    return lo, lo + rng.integers(12, 29, (n_boxes, 3))


def paint(lo, hi):
    grid = torch.full((NV, NV, NV), -1, dtype=torch.int32, device="cuda")
    for k, (l, h) in enumerate(zip(lo, hi)):
        l, h = np.clip(l, 0, NV), np.clip(h, 0, NV)
        grid[l[0]:h[0], l[1]:h[1], l[2]:h[2]] = k
    return grid.reshape(-1)


def cases():
    rng = np.random.default_rng(12)
    lo, hi = boxes(rng, 200)
    a = paint(lo, hi)
    keep = rng.permutation(200)[:180]
    shift = rng.integers(-2, 3, (180, 3))
    lo2, hi2 = boxes(rng, 20)
    b = paint(np.concatenate((lo[keep] + shift, lo2)), np.concatenate((hi[keep] + shift, hi2)))
    yield "boxes", a, b, 200, 200
    x = torch.arange(NV, device="cuda", dtype=torch.int32)
    board = ((x[:, None, None] + x[None, :, None] + x[None, None, :]) % 2).reshape(-1).contiguous()
    yield "checkerboard", board, board.clone(), 2, 2
    g = torch.Generator(device="cuda").manual_seed(5)
    yield "noise", torch.randint(0, 200, (NV ** 3,), generator=g, device="cuda", dtype=torch.int32), \
        torch.randint(0, 200, (NV ** 3,), generator=g, device="cuda", dtype=torch.int32), 200, 200


def probe(name, a, b, n_a, n_b):
    nvox = (NV, NV, NV)
    hip = lambda: object_overlap(a, nvox, b, nvox, (0, 0, 0), n_a, n_b)
    ref = lambda: torch_overlap(a, b, n_a, n_b)
    got, want = hip(), ref()
    for k in ("pair", "in_a", "in_b"):
        assert torch.equal(got[k], want[k]), (name, k)
    t = {"saf_object_overlap": [], "torch_bincount": []}
    for rep in range(REPEATS + 1):  # the first round is the warm-up
        one = {"saf_object_overlap": ms(hip), "torch_bincount": ms(ref)}
        print(rep, name, {k: round(v, 3) for k, v in one.items()}, flush=True)
        if rep:
            for k, v in one.items():
                t[k].append(v)
    out = {"n_a": n_a, "n_b": n_b, "member_share_a": round(float(((a >= 0) & (a < n_a)).float().mean()), 4),
           "member_share_b": round(float(((b >= 0) & (b < n_b)).float().mean()), 4), "pairs_with_shared_voxels": int((got["pair"] > 0).sum()),
           "bytes_read_at_least": 8 * NV ** 3}
    out.update({k: stats(v) for k, v in t.items()})
    out["saf_GBps"] = round(8 * NV ** 3 / out["saf_object_overlap"]["median_ms"] / 1e6, 1)
    out["torch_over_saf"] = round(out["torch_bincount"]["median_ms"] / out["saf_object_overlap"]["median_ms"], 2)
    return out


class _Part(torch.utils.data.Dataset):
    def __init__(self, scan, first, last):
        self.scan, self.first, self.n = scan, first, last - first
        self.imwidth, self.imheight = scan.imwidth, scan.imheight

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return self.scan[self.first + i]


def extend_laps():
    """The scene of tests/test_scene_extend_gpu.py: 32 frames, then 16 more from half a metre further along."""
    from spatially_aware_ai_amd.scene import extend_scene, reconstruct_scene

    scan = syn.SyntheticScan(23, 48, 64, 48, 64)
    for f in scan.frames[32:]:
        f["pose"] = f["pose"].clone()
        f["pose"][0, :3, 3] += torch.tensor([0.5, -0.4, 0.0])
    names, colors = syn.scene_class_names(), syn.scene_class_colors()
    config = {"voxel_size": 0.08, "trunc_vox": 3, "clip_patch_size": scan.patch, "clip_patch_stride": scan.stride}
    out = {}
    for rep in range(2):  # the second round is the one reported
        clip, seg = syn.ReplayClip(scan, class_names=names), syn.ReplaySeg(scan)
        first = reconstruct_scene(_Part(scan, 0, 32), config, clip, seg, names, colors)
        res = extend_scene(first, _Part(scan, 32, 48), config, clip, seg, names, colors, keep_identities=True)
        m = res.object_matches
        out = {"nvox": [int(v) for v in res.fusion.nvox], "objects_before": len(first.scene_knowledge["unique_objects"]),
               "objects_after": len(res.scene_knowledge["unique_objects"]),
               "matches": {k: len(getattr(m, k)) for k in ("kept", "absorbed", "moved", "new", "missing", "class_changed")},
               "seconds": {k: round(v, 5) for k, v in res.seconds.items() if not isinstance(v, dict)}}
    return out


if __name__ == "__main__":
    res = {"device": torch.cuda.get_device_name(0), "grid": NV, "repeats": REPEATS}
    for name, a, b, n_a, n_b in cases():
        res[name] = probe(name, a, b, n_a, n_b)
        del a, b
        torch.cuda.empty_cache()
    res["extend_scene_test_scene"] = extend_laps()
    if len(sys.argv) > 1:
        json.dump(res, open(sys.argv[1], "w"), indent=1)
    print(json.dumps(res))
