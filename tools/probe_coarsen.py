"""256^3 x 512 f32 fused from 128 frames -- the coherent scene bench.py uses (depth B), then random depth (A: four voxels in five
touched) -- coarsened by 2 into a prepared 128^3 volume.  Taken alternately, five repetitions after a warm-up, device times by HIP
events: the pass alone (saf_volume_coarsen), a torch restatement of the same weighted mean on the device (the fine volume viewed as
[X, 2, Y, 2, Z, 2], masks from the counts, the pass's formulas one operation at a time over the eight children in order, 8 coarse
x-planes at a time so that its temporaries stay near 3 GB -- the only other way there is), and saf_volume_carry of the same source
into a prepared volume of its own size as the copy-rate yardstick.  Bytes by the accounting of include/saf.h.  Nothing else may
run on the GPU; about 80 GB of device memory are in use.
Usage: python tools/probe_coarsen.py [out.json]   (profiles/r16/coarsen.json is its output)."""
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
W, H, DIM, NF, NV, F = 640, 480, 512, 128, 256, 2
NC = NV // F
SMALL = ("tsdf", "tsdf_weight", "weight", "rgb")
NAMES = SMALL + ("clip_feat",)
SLAB = 8  # coarse x-planes per step of the torch restatement


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


def torch_coarsen(src, dst):
    """The weighted mean with torch, per slab of coarse x-planes.  (It also writes zero rows where no child contributes.)"""
    fine = lambda t: t.view(NV, NV, NV, *t.shape[1:])
    coarse = lambda t: t.view(NC, NC, NC, *t.shape[1:])
    for x0 in range(0, NC, SLAB):
        def kids(t):  # [SLAB, NC, NC, F, F, F, ...]: a view
            v = fine(t)[F * x0:F * (x0 + SLAB)]
            v = v.view(SLAB, F, NC, F, NC, F, *v.shape[3:])
            return v.permute(0, 2, 4, 1, 3, 5, *range(6, v.dim()))

        for w_name, names in (("tsdf_weight", ("tsdf",)), ("weight", ("rgb", "clip_feat"))):
            w = kids(src[w_name])
            pos = w > 0
            k = pos.sum(dim=(3, 4, 5))
            r = 1.0 / torch.where(k >= 2, (w * pos).sum(dim=(3, 4, 5)), 1).float()
            for name in names:
                x = kids(src[name])
                acc = one = None
                started = torch.zeros_like(k, dtype=torch.bool)
                for c in range(F ** 3):
                    cx, cy, cz = c // (F * F), c // F % F, c % F
                    xc = x[:, :, :, cx, cy, cz]
                    e = (...,) + (None,) * (xc.dim() - 3)
                    on = pos[:, :, :, cx, cy, cz]
                    p = xc * (w[:, :, :, cx, cy, cz].float() * r)[e]
                    if acc is None:
                        acc, one = torch.where(on[e], p, 0.0), torch.where(on[e], xc, 0.0)
                    else:
                        acc = torch.where(on[e], torch.where(started[e], acc + p, p), acc)
                        one = torch.where((on & ~started)[e], xc, one)
                    started |= on
                e = (...,) + (None,) * (acc.dim() - 3)
                coarse(dst[name])[x0:x0 + SLAB] = torch.where((k >= 2)[e], acc, one)
            coarse(dst[w_name])[x0:x0 + SLAB] = (w * pos).amax(dim=(3, 4, 5))


def probe(depth_kind):
    npy, npx = syn.feature_map_shape(W, H)
    grid = syn.make_grid(NV)
    fz = ClipFusion(grid.origin, grid.voxel_size, grid.nvox, grid.trunc, False, FakeClip(), None, 10, 10, keep_xyz_world=False,
                    defer_frames=False, device="cuda").cuda()
    fz.integrate_features(*gen_frames_gpu(NF, W, H, DIM, npy, npx, depth_kind, 2024, "cuda"))
    fz.flush()
    src = {k: getattr(fz, k) for k in NAMES}  # (attribute access: the rows of untouched voxels are zero)
    n, nc = NV ** 3, NC ** 3
    kids = lambda t: t.view(NC, F, NC, F, NC, F)
    k_rows, k_tsdf = (kids(src["weight"]) > 0).sum(dim=(1, 3, 5)), (kids(src["tsdf_weight"]) > 0).sum(dim=(1, 3, 5))
    m_src, t_src = int((src["weight"] > 0).sum()), int((src["tsdf_weight"] > 0).sum())
    rb, rc, tb, tc = int((k_rows >= 2).sum()), int((k_rows == 1).sum()), int((k_tsdf >= 2).sum()), int((k_tsdf == 1).sum())
    row = DIM * 4
    # include/saf.h: 8 N_src of counts read, 12 / 4 more per fine voxel with weight / tsdf_weight > 0, one row per contributing child;
    # 28 N_dst written, one row per coarse voxel with K >= 1
    coarsen_bytes = 8 * n + 12 * m_src + 4 * t_src + m_src * row + 28 * nc + (rb + rc) * row
    carry_bytes = 2 * (28 * n + m_src * row)
    out = {"depth_kind": depth_kind, "touched_share_fine": round(m_src / n, 4), "touched_share_coarse": round((rb + rc) / nc, 4),
           "rows_read": m_src, "rows_blended": rb, "rows_copied": rc, "tsdf_blended": tb, "tsdf_copied": tc,
           "mean_children_per_written_row": round(m_src / max(rb + rc, 1), 3), "coarsen_bytes": coarsen_bytes, "carry_bytes": carry_bytes}
    zeros = lambda k, cnt: torch.zeros((cnt,) + tuple(src[k].shape[1:]), dtype=src[k].dtype, device="cuda")
    dst = {k: zeros(k, nc) for k in NAMES}
    dst_t = {k: zeros(k, nc) for k in NAMES}
    big = {k: zeros(k, n) for k in SMALL}
    big["clip_feat"] = torch.empty_like(src["clip_feat"])
    p = _abi.ptr
    vs = fz._c_volume(for_fuse=True)
    desc = lambda v, m: _abi.SafVolume(m, m, m, DIM, 0, _abi.SAF_F32, 0, vs.trunc, vs.axis_x, vs.axis_y, vs.axis_z, p(v["tsdf"]),
                                       p(v["tsdf_weight"]), p(v["weight"]), p(v["rgb"]), p(v["clip_feat"]), None)
    vd, vc = desc(dst, NC), desc(big, NV)
    stream = torch.cuda.current_stream().cuda_stream
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")

    def pass_only():
        check(lib().saf_volume_coarsen(C.byref(vs), C.byref(vd), F, 0, 0, 0, p(counts), stream), "saf_volume_coarsen")

    def carry_only():
        check(lib().saf_volume_carry(C.byref(vs), C.byref(vc), 0, 0, 0, None, None, None, stream), "saf_volume_carry")

    t = {"coarsen_pass": [], "torch_restatement": [], "carry_pass": []}
    for rep in range(REPEATS + 1):  # the first round is the warm-up
        got = {}
        counts.zero_()
        got["coarsen_pass"] = ms(pass_only)
        if rep == 0:
            assert counts.tolist() == [rb, rc, tb, tc], (counts.tolist(), [rb, rc, tb, tc])
        got["torch_restatement"] = ms(lambda: torch_coarsen(src, dst_t))
        if rep == 0:  # (recorded, not asserted: the restatement is a yardstick for time)
            out["torch_equals_pass"] = {k: bool(torch.equal(dst_t[k], dst[k])) for k in NAMES}
            out["torch_max_abs_diff_clip_feat"] = float((dst_t["clip_feat"] - dst["clip_feat"]).abs().max())
        got["carry_pass"] = ms(carry_only)
        print(rep, depth_kind, {k: round(v, 2) for k, v in got.items()}, flush=True)
        if rep:
            for k, v in got.items():
                t[k].append(v)
    out.update({k: stats(v) for k, v in t.items()})
    out["coarsen_TBps"] = round(coarsen_bytes / out["coarsen_pass"]["median_ms"] / 1e9, 3)
    out["carry_TBps"] = round(carry_bytes / out["carry_pass"]["median_ms"] / 1e9, 3)
    out["coarsen_rate_over_carry_rate"] = round(out["coarsen_TBps"] / out["carry_TBps"], 3)
    out["torch_over_coarsen_pass"] = round(out["torch_restatement"]["median_ms"] / out["coarsen_pass"]["median_ms"], 2)
    out["coarsen_pass_over_carry_pass"] = round(out["coarsen_pass"]["median_ms"] / out["carry_pass"]["median_ms"], 2)
    return out


if __name__ == "__main__":
    res = {"device": torch.cuda.get_device_name(0), "grid": NV, "feat_dim": DIM, "frames": NF, "factor": F, "repeats": REPEATS,
           "coherent_scene": probe("B")}
    if len(sys.argv) > 1:  # (kept as soon as it exists)
        json.dump(res, open(sys.argv[1], "w"), indent=1)
    torch.cuda.empty_cache()
    res["random_depth"] = probe("A")
    if len(sys.argv) > 1:
        json.dump(res, open(sys.argv[1], "w"), indent=1)
    print(json.dumps(res))
