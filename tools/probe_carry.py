"""256^3 x 512 f32, fused from the coherent scene bench.py uses (depth B) and from random depth (A: four voxels in five touched):
``move_grid`` by (16, -8, 4) voxels into a box of the same size, beside the same move done with torch slice assignments
(``dst.view(nx, ny, nz, ...)[box] = src.view(...)[box]`` per buffer) -- the only way there was before saf_volume_carry.
Device times by HIP events, five repetitions each, taken alternately; nothing else may run on the GPU.
Usage: python tools/probe_carry.py [out.json]   (profiles/r11/carry.json is its output)."""
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import gen_frames_gpu
from spatially_aware_ai_amd import ClipFusion, _abi
from spatially_aware_ai_amd import synthetic as syn
from spatially_aware_ai_amd._lib import check, lib

REPEATS = 5
W, H, DIM, NF, NV = 640, 480, 512, 128, 256
SHIFT = (16, -8, 4)
SMALL = ("tsdf", "tsdf_weight", "weight", "rgb")


class FakeClip:
    feature_dim = DIM


def ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(v):
    s = sorted(v)
    return {"ms": [round(x, 3) for x in v], "median_ms": round(s[len(s) // 2], 3), "spread_ms": round(s[-1] - s[0], 3)}


def boxes():
    d = tuple(slice(max(0, -o), min(NV, NV - o)) for o in SHIFT)
    return d, tuple(slice(s.start + o, s.stop + o) for s, o in zip(d, SHIFT))


def torch_move(src, dst):
    """The move with slice assignments into prepared buffers (the zeroing of ``dst`` is timed apart)."""
    d, s = boxes()
    for name in SMALL + ("clip_feat",):
        a, b = src[name], dst[name]
        b.view(NV, NV, NV, *b.shape[1:])[d] = a.view(NV, NV, NV, *a.shape[1:])[s]


def probe(depth_kind):
    npy, npx = syn.feature_map_shape(W, H)
    grid = syn.make_grid(NV)
    fz = ClipFusion(grid.origin, grid.voxel_size, grid.nvox, grid.trunc, False, FakeClip(), None, 10, 10, keep_xyz_world=False,
                    defer_frames=False, device="cuda").cuda()
    fz.integrate_features(*gen_frames_gpu(NF, W, H, DIM, npy, npx, depth_kind, 2024, "cuda"))
    fz.flush()
    n = NV ** 3
    src = dict(fz._buffers)
    d, s = boxes()
    n_overlap = 1
    for sl in d:
        n_overlap *= sl.stop - sl.start
    touched = int((src["weight"] > 0).sum())
    moved_rows = int((src["weight"].view(NV, NV, NV)[s] > 0).sum())
    out = {"depth_kind": depth_kind, "touched_share": round(touched / n, 4), "overlap_voxels": n_overlap, "rows_carried": moved_rows,
           # include/saf.h: 28 N_overlap + M row_bytes, read and written; the slice copies: N_overlap (28 + row_bytes), read and written
           "carry_bytes_each_way": 28 * n_overlap + moved_rows * DIM * 4, "slice_copy_bytes_each_way": n_overlap * (28 + DIM * 4)}
    dst = {k: torch.zeros_like(src[k]) for k in SMALL}
    dst["clip_feat"] = torch.empty_like(src["clip_feat"])
    vs = fz._c_volume(for_fuse=True)
    p = _abi.ptr
    vd = _abi.SafVolume(NV, NV, NV, DIM, 0, _abi.SAF_F32, 0, vs.trunc, vs.axis_x, vs.axis_y, vs.axis_z, p(dst["tsdf"]), p(dst["tsdf_weight"]),
                        p(dst["weight"]), p(dst["rgb"]), p(dst["clip_feat"]), None)
    stream = torch.cuda.current_stream().cuda_stream

    def carry_only():
        check(lib().saf_volume_carry(C.byref(vs), C.byref(vd), SHIFT[0], SHIFT[1], SHIFT[2], None, None, None, stream), "saf_volume_carry")

    def move_grid():
        fz.move_grid(SHIFT, (NV, NV, NV))

    def put_back():  # the module holds the fused box again (the moved buffers go back to the allocator)
        fz._buffers.update(src)
        fz.index_offset = (0, 0, 0)
        fz.__dict__["_feat_stale"] = False

    t = {"move_grid": [], "carry_pass": [], "torch_slices": [], "torch_zero_clip_feat": []}
    for rep in range(REPEATS + 1):  # the first round is the warm-up
        got = {"move_grid": ms(move_grid)}
        if rep == 0:  # what the moved module holds is what the slice copies give, where the old box reaches
            want = {k: torch.zeros_like(src[k]) for k in SMALL + ("clip_feat",)}
            torch_move(src, want)
            for k in SMALL + ("clip_feat",):
                assert torch.equal(getattr(fz, k), want[k]), k
            del want
        put_back()
        got["carry_pass"] = ms(carry_only)
        got["torch_slices"] = ms(lambda: torch_move(src, dst))
        got["torch_zero_clip_feat"] = ms(lambda: dst["clip_feat"].zero_())
        print(rep, depth_kind, {k: round(v, 2) for k, v in got.items()}, flush=True)
        if rep:
            for k, v in got.items():
                t[k].append(v)
    out.update({k: stats(v) for k, v in t.items()})
    out["torch_over_move_grid"] = round(out["torch_slices"]["median_ms"] / out["move_grid"]["median_ms"], 2)
    out["carry_GBps"] = round(2 * out["carry_bytes_each_way"] / out["carry_pass"]["median_ms"] / 1e6, 1)
    out["torch_GBps"] = round(2 * out["slice_copy_bytes_each_way"] / out["torch_slices"]["median_ms"] / 1e6, 1)
    return out


if __name__ == "__main__":
    res = {"device": torch.cuda.get_device_name(0), "grid": NV, "feat_dim": DIM, "frames": NF, "shift": SHIFT, "repeats": REPEATS,
           "coherent_scene": probe("B")}
    torch.cuda.empty_cache()
    res["random_depth"] = probe("A")
    if len(sys.argv) > 1:
        json.dump(res, open(sys.argv[1], "w"), indent=1)
    print(json.dumps(res))
