"""256^3 x 512 f32: two volumes of one lattice, the second shifted by (16, -8, 4) voxels, each fused from 128 frames -- the coherent
scene bench.py uses (depth B), then random depth (A: four voxels in five touched) -- and the first absorbs the second over their
overlap.  Taken alternately, five repetitions after a warm-up, device times by HIP events: ``absorb(grow=False)``, the pass alone
(saf_volume_absorb), a torch restatement of the same blend on the device (sliced views, ``torch.where`` on the weights, the same
formulas, into the same buffers, 32 x-planes at a time so that its temporaries stay at 4 GB -- the only way there was), and
saf_volume_carry over the same boxes into a prepared volume as the copy-rate yardstick.  The absorbing volume is put back from a
copy before every candidate (not timed).  Nothing else may run on the GPU; about 170 GB of device memory are in use.
Usage: python tools/probe_absorb.py [out.json]   (profiles/r13/absorb.json is its output)."""
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
SHIFT = (16, -8, 4)  # the second volume's index offset; the first one's is 0
SMALL = ("tsdf", "tsdf_weight", "weight", "rgb")
NAMES = SMALL + ("clip_feat",)
SLAB = 32


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
    """(slices into the absorbing volume, slices into the absorbed one): destination index + SHIFT's negative = source index."""
    off = tuple(-o for o in SHIFT)  # off = self.index_offset - other.index_offset
    d = tuple(slice(max(0, -o), min(NV, NV - o)) for o in off)
    return d, tuple(slice(s.start + o, s.stop + o) for s, o in zip(d, off)), off


def torch_absorb(src, dst):
    """The blend with torch: per slab of x-planes, masks from the four weight arrays, the pass's formulas one operation at a time."""
    d, s, _ = boxes()
    g = lambda t: t.view(NV, NV, NV, *t.shape[1:])
    for x0 in range(d[0].start, d[0].stop, SLAB):
        x1 = min(x0 + SLAB, d[0].stop)
        dd = (slice(x0, x1),) + d[1:]
        ss = (slice(x0 - d[0].start + s[0].start, x1 - d[0].start + s[0].start),) + s[1:]
        for w_name, names in (("tsdf_weight", ("tsdf",)), ("weight", ("rgb", "clip_feat"))):
            ws, wd = g(src[w_name])[ss], g(dst[w_name])[dd]
            copy, blend = (ws > 0) & (wd <= 0), (ws > 0) & (wd > 0)
            w = wd + ws
            r = 1.0 / torch.where(blend, w, 1).float()
            cs, cd = ws.float() * r, wd.float() * r
            for name in names:
                xs, xd = g(src[name])[ss], g(dst[name])[dd]
                e = (...,) + (None,) * (xs.dim() - 3)
                mixed = xs * cs[e] + xd * cd[e]
                g(dst[name])[dd] = torch.where(blend[e], mixed, torch.where(copy[e], xs, xd))
            g(dst[w_name])[dd] = torch.where(blend, w, torch.where(copy, ws, wd))


def fused(depth_kind, seed, index_offset):
    npy, npx = syn.feature_map_shape(W, H)
    grid = syn.make_grid(NV)
    fz = ClipFusion(grid.origin, grid.voxel_size, grid.nvox, grid.trunc, False, FakeClip(), None, 10, 10, keep_xyz_world=False,
                    defer_frames=False, index_offset=index_offset, device="cuda").cuda()
    fz.integrate_features(*gen_frames_gpu(NF, W, H, DIM, npy, npx, depth_kind, seed, "cuda"))
    fz.flush()
    return fz


def probe(depth_kind):
    fz, other = fused(depth_kind, 2024, (0, 0, 0)), fused(depth_kind, 2025, SHIFT)
    n = NV ** 3
    mine, src = fz._buffers, other._buffers
    keep = {k: mine[k].clone() for k in NAMES}  # the absorbing volume as fused: put back before every candidate
    d, s, off = boxes()
    n_overlap = 1
    for sl in d:
        n_overlap *= sl.stop - sl.start
    g = lambda t: t.view(NV, NV, NV)
    ws, wd, tws, twd = g(src["weight"])[s], g(mine["weight"])[d], g(src["tsdf_weight"])[s], g(mine["tsdf_weight"])[d]
    rb, rc = int(((ws > 0) & (wd > 0)).sum()), int(((ws > 0) & (wd <= 0)).sum())
    tb, tc = int(((tws > 0) & (twd > 0)).sum()), int(((tws > 0) & (twd <= 0)).sum())
    row = DIM * 4
    # include/saf.h: 28 N_overlap read from each volume; a copied row: one read, one written; a blended row: two read, one written;
    # the small fields written: 16 bytes per voxel the feature side writes, 8 per voxel the TSDF side writes
    absorb_bytes = 56 * n_overlap + (2 * rc + 3 * rb) * row + 16 * (rc + rb) + 8 * (tc + tb)
    carried = int((ws > 0).sum())
    carry_bytes = 2 * (28 * n_overlap + carried * row)
    out = {"depth_kind": depth_kind, "touched_share_self": round(int((mine["weight"] > 0).sum()) / n, 4),
           "touched_share_other": round(int((src["weight"] > 0).sum()) / n, 4), "overlap_voxels": n_overlap, "rows_blended": rb,
           "rows_copied": rc, "tsdf_blended": tb, "tsdf_copied": tc, "absorb_bytes": absorb_bytes, "carry_bytes": carry_bytes,
           "bytes_per_touched_row_over_carry": round((absorb_bytes / max(rb + rc, 1)) / (carry_bytes / max(carried, 1)), 3)}
    vs, vd = other._c_volume(for_fuse=True), fz._c_volume(for_fuse=True)
    scratch = {k: torch.zeros_like(mine[k]) for k in SMALL}
    scratch["clip_feat"] = torch.empty_like(mine["clip_feat"])
    p = _abi.ptr
    vc = _abi.SafVolume(NV, NV, NV, DIM, 0, _abi.SAF_F32, 0, vs.trunc, vs.axis_x, vs.axis_y, vs.axis_z, p(scratch["tsdf"]),
                        p(scratch["tsdf_weight"]), p(scratch["weight"]), p(scratch["rgb"]), p(scratch["clip_feat"]), None)
    stream = torch.cuda.current_stream().cuda_stream
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")

    def put_back():
        for k in NAMES:
            mine[k].copy_(keep[k])

    def pass_only():
        check(lib().saf_volume_absorb(C.byref(vs), C.byref(vd), off[0], off[1], off[2], p(counts), stream), "saf_volume_absorb")

    def carry_only():
        check(lib().saf_volume_carry(C.byref(vs), C.byref(vc), off[0], off[1], off[2], None, None, None, stream), "saf_volume_carry")

    t = {"absorb": [], "absorb_pass": [], "torch_restatement": [], "carry_pass": []}
    for rep in range(REPEATS + 1):  # the first round is the warm-up
        got = {}
        put_back()
        got["absorb"] = ms(lambda: fz.absorb(other, grow=False))
        put_back()
        counts.zero_()
        got["absorb_pass"] = ms(pass_only)
        if rep == 0:
            assert counts.tolist() == [rb, rc, tb, tc], (counts.tolist(), [rb, rc, tb, tc])
            want = scratch  # (the yardstick's destination holds the pass's result for the comparison below: no sixth volume)
            for k in NAMES:
                want[k].copy_(mine[k])
        put_back()
        got["torch_restatement"] = ms(lambda: torch_absorb(src, mine))
        if rep == 0:  # (recorded, not asserted: the restatement is a yardstick for time)
            out["torch_equals_pass"] = {k: bool(torch.equal(mine[k], want[k])) for k in NAMES}
            out["torch_max_abs_diff_clip_feat"] = float((mine["clip_feat"] - want["clip_feat"]).abs().max())
            for k in SMALL:
                scratch[k].zero_()
        got["carry_pass"] = ms(carry_only)
        print(rep, depth_kind, {k: round(v, 2) for k, v in got.items()}, flush=True)
        if rep:
            for k, v in got.items():
                t[k].append(v)
    out.update({k: stats(v) for k, v in t.items()})
    out["absorb_TBps"] = round(absorb_bytes / out["absorb_pass"]["median_ms"] / 1e9, 3)
    out["carry_TBps"] = round(carry_bytes / out["carry_pass"]["median_ms"] / 1e9, 3)
    out["absorb_rate_over_carry_rate"] = round(out["absorb_TBps"] / out["carry_TBps"], 3)
    out["torch_over_absorb_pass"] = round(out["torch_restatement"]["median_ms"] / out["absorb_pass"]["median_ms"], 2)
    out["absorb_pass_over_carry_pass"] = round(out["absorb_pass"]["median_ms"] / out["carry_pass"]["median_ms"], 2)
    return out


if __name__ == "__main__":
    res = {"device": torch.cuda.get_device_name(0), "grid": NV, "feat_dim": DIM, "frames_each": NF, "shift": SHIFT, "repeats": REPEATS,
           "coherent_scene": probe("B")}
    if len(sys.argv) > 1:  # (kept as soon as it exists)
        json.dump(res, open(sys.argv[1], "w"), indent=1)
    torch.cuda.empty_cache()
    res["random_depth"] = probe("A")
    if len(sys.argv) > 1:
        json.dump(res, open(sys.argv[1], "w"), indent=1)
    print(json.dumps(res))
