"""The NumPy float32 statement of saf_volume_coarsen (include/saf.h) that the tests of ``coarsen`` hold the device pass to.

A volume is a dict of arrays shaped by its grid, as in carry_reference.py and absorb_reference.py: ``tsdf`` f32, ``tsdf_weight``,
``weight`` i32 [nx,ny,nz], ``rgb`` f32 [nx,ny,nz,3], ``clip_feat`` [nx,ny,nz,D] and optionally ``labels_one_hot`` i32 [nx,ny,nz,C].
``kind`` names the element type of ``clip_feat``: "f32", or "bf16" / "f16" (np.int16 bit patterns), widened and narrowed by
absorb_reference's helpers.  The fine box holds its voxels from global index ``off`` of its lattice; global coarse voxel I covers
the fine global indices f I .. f I + f - 1.  Every f32 operation of the device pass is one NumPy float32 operation here, in the
same order (children in ascending fine flat index), so every comparison against it is exact -- as long as no NaN is computed WITH.
``mean64`` is the float64 weighted mean the error bounds are stated against."""
import numpy as np

from absorb_reference import narrow, widen

F32 = np.float32


def mapping(off, nvox, f):
    """(index_offset', nvox', lead) per axis: floor(off / f), ceil((off + n) / f) - floor(off / f), and how many children of the
    first block lie below the fine box (off - f floor(off / f), in 0 .. f - 1)."""
    off, nvox = [int(v) for v in off], [int(v) for v in nvox]
    new_off = [o // f for o in off]
    new_n = [-((-(o + n)) // f) - o // f for o, n in zip(off, nvox)]
    return tuple(new_off), tuple(new_n), tuple(o - f * q for o, q in zip(off, new_off))


def coarse_origin(origin, voxel_size, f):
    """origin' = origin + 0.5 (f - 1) vs in float64: the centre of the block of global coarse index 0."""
    return np.asarray(origin, dtype=np.float64) + 0.5 * (f - 1) * float(voxel_size)


def children(a, off, f, fill=0):
    """``a`` [nx,ny,nz,...] as [nx',ny',nz', f^3, ...]: the children of every coarse voxel in ascending fine flat index (x slowest,
    z fastest); ``fill`` where a child lies outside the fine box."""
    _, new_n, lead = mapping(off, a.shape[:3], f)
    tail = a.shape[3:]
    pad = np.full(tuple(f * n for n in new_n) + tail, fill, dtype=a.dtype)
    pad[lead[0]:lead[0] + a.shape[0], lead[1]:lead[1] + a.shape[1], lead[2]:lead[2] + a.shape[2]] = a
    pad = pad.reshape((new_n[0], f, new_n[1], f, new_n[2], f) + tail)
    pad = np.moveaxis(pad, (1, 3, 5), (3, 4, 5))  # [nx',ny',nz', f,f,f, ...]
    return np.ascontiguousarray(pad).reshape(tuple(new_n) + (f ** 3,) + tail)


def counts_of(w):
    """(K, W, max) over the last axis of the children's counts: contributing children, their int32 sum, their maximum."""
    pos = w > 0
    return pos.sum(-1).astype(np.int32), np.where(pos, w, 0).sum(-1, dtype=np.int32), np.where(pos, w, 0).max(-1).astype(np.int32)


def blend(x, w):
    """The K >= 2 case on children's values ``x`` [..., f^3, C] (float32) and counts ``w`` [..., f^3]: r = 1 / (float)W,
    c_k = (float)w_k * r, acc = x_1 * c_1, acc = acc + x_k * c_k.  Where K < 2 the result means nothing."""
    pos = w > 0
    _, total, _ = counts_of(w)
    with np.errstate(all="ignore"):
        r = F32(1.0) / np.maximum(total, 1).astype(F32)
        acc = np.zeros(x.shape[:-2] + x.shape[-1:], dtype=F32)
        started = np.zeros(w.shape[:-1], dtype=bool)
        for c in range(w.shape[-1]):
            on = pos[..., c]
            if not on.any():
                continue
            ck = (w[..., c].astype(F32) * r).astype(F32)
            p = (x[..., c, :].astype(F32) * ck[..., None]).astype(F32)
            s = (acc + p).astype(F32)
            new = np.where(started[..., None], s, p)
            acc = np.where(on[..., None], new, acc)
            started |= on
    return acc


def only_child(raw, w):
    """The K == 1 case: the bytes of the one contributing child of ``raw`` [..., f^3, C] (any dtype).  Where K != 1: the first
    contributing child's, or child 0's."""
    first = np.argmax(w > 0, axis=-1)
    return np.take_along_axis(raw, first[..., None, None], axis=-2)[..., 0, :]


def mean64(x, w):
    """The float64 weighted mean over the contributing children of ``x`` [..., f^3, C]; NaN where no child contributes."""
    pos = w > 0
    wx = np.where(pos[..., None], x.astype(np.float64) * np.where(pos, w, 0).astype(np.float64)[..., None], 0.0)
    with np.errstate(all="ignore"):
        return wx.sum(-2) / np.where(pos, w, 0).astype(np.float64).sum(-1)[..., None]


def coarsen(src, off, f, kind="f32", dst=None):
    """The coarse volume and (rows blended, rows copied, tsdf voxels blended, tsdf voxels copied).  ``dst``: what the destination
    held before -- its feature and label rows stay where no child contributes (default: zeros); the small fields are written
    everywhere.  No value of a child with count 0 is used."""
    _, new_n, _ = mapping(off, src["weight"].shape, f)
    w, tw = children(src["weight"], off, f), children(src["tsdf_weight"], off, f)
    k, _, wmax = counts_of(w)
    kt, _, tmax = counts_of(tw)
    out = {"weight": wmax, "tsdf_weight": tmax}
    sel = lambda kk, one, many, none: np.where((kk == 1)[..., None], one, np.where((kk >= 2)[..., None], many, none))
    # ---- the TSDF side
    t = children(src["tsdf"], off, f)[..., None]
    out["tsdf"] = sel(kt, only_child(t, tw), blend(t, tw), F32(0))[..., 0].astype(F32)
    # ---- the feature side
    c = children(src["rgb"], off, f)
    out["rgb"] = sel(k, only_child(c, w), blend(c, w), F32(0)).astype(F32)
    rows = children(src["clip_feat"], off, f)
    keep = np.zeros(new_n + rows.shape[-1:], dtype=rows.dtype) if dst is None else dst["clip_feat"]
    out["clip_feat"] = sel(k, only_child(rows, w), narrow(blend(widen(rows, kind), w), kind), keep).astype(rows.dtype)
    if "labels_one_hot" in src:
        lab = children(src["labels_one_hot"], off, f)
        keep = np.zeros(new_n + lab.shape[-1:], dtype=np.int32) if dst is None else dst["labels_one_hot"]
        total = np.where((w > 0)[..., None], lab, 0).sum(-2, dtype=np.int32)
        out["labels_one_hot"] = np.where((k >= 1)[..., None], total, keep).astype(np.int32)
    return out, (int((k >= 2).sum()), int((k == 1).sum()), int((kt >= 2).sum()), int((kt == 1).sum()))


def child_counts(src, off, f):
    """(K of the feature side, K of the TSDF side) per coarse voxel."""
    return counts_of(children(src["weight"], off, f))[0], counts_of(children(src["tsdf_weight"], off, f))[0]
