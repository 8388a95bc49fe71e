"""The NumPy float32 statement of saf_volume_absorb (include/saf.h) that the tests of ``absorb`` hold the device pass to, with slices.

A volume is a dict of arrays shaped by its grid, as in carry_reference.py: ``tsdf`` f32, ``tsdf_weight``, ``weight`` i32 [nx,ny,nz],
``rgb`` f32 [nx,ny,nz,3], ``clip_feat`` [nx,ny,nz,D] and optionally ``labels_one_hot`` i32 [nx,ny,nz,C].  ``kind`` names the element
type of ``clip_feat``: "f32" (an np.float32 array), or "bf16" / "f16" (an np.int16 array of bit patterns: NumPy has no bfloat16).
16-bit rows are widened and narrowed by torch's CPU conversions (exact; one round-to-nearest-even).  Destination voxel (x, y, z)
corresponds to source voxel (x + off).  Every f32 operation of the device pass is one NumPy float32 operation here, in the same
order, so every comparison against it is exact -- as long as no NaN is computed WITH (payloads are the hardware's own)."""
import numpy as np
import torch

from carry_reference import overlap

TORCH_16 = {"bf16": torch.bfloat16, "f16": torch.float16}


def widen(a, kind):
    """float32 values of feature elements."""
    if kind == "f32":
        return np.asarray(a, dtype=np.float32)
    return torch.from_numpy(np.ascontiguousarray(a)).view(TORCH_16[kind]).float().numpy()


def narrow(x, kind):
    """Feature elements of float32 values: one rounding to nearest-even."""
    if kind == "f32":
        return np.asarray(x, dtype=np.float32)
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(TORCH_16[kind]).view(torch.int16).numpy()


def coefficients(ws, wd):
    """(cs, cd, w') of a blend of counts ws, wd > 0 (int32 arrays): r = 1 / (float)w' by IEEE division."""
    w = (wd + ws).astype(np.int32)
    r = np.float32(1.0) / w.astype(np.float32)
    return ws.astype(np.float32) * r, wd.astype(np.float32) * r, w


def mix(xs, xd, cs, cd):
    """x' = xs * cs + xd * cd: two rounded products, one rounded sum."""
    ps = (xs * cs).astype(np.float32)
    pd = (xd * cd).astype(np.float32)
    return (ps + pd).astype(np.float32)


def states(ws, wd):
    """(copied, blended) for the counts of one side."""
    return (ws > 0) & (wd <= 0), (ws > 0) & (wd > 0)


def absorb(src, dst, off, kind="f32"):
    """``dst`` (modified in place) after the pass, and (rows blended, rows copied, tsdf voxels blended, tsdf voxels copied).  No row
    of ``src`` with weight 0 is read, no row of ``dst`` with weight 0 is read; where the source's count is 0 nothing is written."""
    ov = overlap(src["weight"].shape, dst["weight"].shape, off)
    if ov is None:
        return dst, (0, 0, 0, 0)
    d, s = ov
    # ---- the TSDF side
    ws, wd = src["tsdf_weight"][s], dst["tsdf_weight"][d].copy()
    t_copy, t_blend = states(ws, wd)
    cs, cd, w = coefficients(ws[t_blend], wd[t_blend])
    tsdf, tw = dst["tsdf"][d], dst["tsdf_weight"][d]  # (basic slices: views)
    tsdf[t_blend] = mix(src["tsdf"][s][t_blend], tsdf[t_blend], cs, cd)
    tsdf[t_copy] = src["tsdf"][s][t_copy]
    tw[t_blend] = w
    tw[t_copy] = ws[t_copy]
    # ---- the feature side
    ws, wd = src["weight"][s], dst["weight"][d].copy()
    copy, blend = states(ws, wd)
    cs, cd, w = coefficients(ws[blend], wd[blend])
    rgb, wt, feat = dst["rgb"][d], dst["weight"][d], dst["clip_feat"][d]
    rgb[blend] = mix(src["rgb"][s][blend], rgb[blend], cs[:, None], cd[:, None])
    rgb[copy] = src["rgb"][s][copy]
    feat[blend] = narrow(mix(widen(src["clip_feat"][s][blend], kind), widen(feat[blend], kind), cs[:, None], cd[:, None]), kind)
    feat[copy] = src["clip_feat"][s][copy]
    if "labels_one_hot" in src:
        lab = dst["labels_one_hot"][d]
        lab[blend] = lab[blend] + src["labels_one_hot"][s][blend]
        lab[copy] = src["labels_one_hot"][s][copy]
    wt[blend] = w
    wt[copy] = ws[copy]
    return dst, (int(blend.sum()), int(copy.sum()), int(t_blend.sum()), int(t_copy.sum()))


def written_masks(src, dst, off):
    """Boolean [nx,ny,nz] masks over the destination, from the volumes BEFORE the pass: ``inside`` (the overlap), ``copy`` / ``blend``
    (the feature side's two writing states) and ``t_copy`` / ``t_blend`` (the TSDF side's)."""
    shape = dst["weight"].shape
    m = {k: np.zeros(shape, dtype=bool) for k in ("inside", "copy", "blend", "t_copy", "t_blend")}
    ov = overlap(src["weight"].shape, shape, off)
    if ov is not None:
        d, s = ov
        m["inside"][d] = True
        m["copy"][d], m["blend"][d] = states(src["weight"][s], dst["weight"][d])
        m["t_copy"][d], m["t_blend"][d] = states(src["tsdf_weight"][s], dst["tsdf_weight"][d])
    return m
