"""NumPy restatement of free-space carving (include/saf.h: saf_free_space_observe, saf_volume_carve) for the tests:
the erosion of the depth, the evidence from the ORACLE's per-frame classification (oracle.OracleVolume.classify: bit 0 = valid,
bit 1 = tsdf_valid), the decision, and the carved volume.  Nothing here calls the code under test."""
import numpy as np
import torch

NAMES = ("tsdf", "tsdf_weight", "weight", "rgb", "clip_feat", "labels_one_hot")


def erode(depth, e):
    """[B,H,W] or [H,W] float32: ``e == 0`` unchanged; else the minimum over the (2e+1)^2 window clipped at the border if every
    pixel of that window is finite and > 0, else 0."""
    d = np.asarray(depth, dtype=np.float32)
    if e == 0:
        return d.copy()
    flat = d.reshape((-1,) + d.shape[-2:])
    h, w = flat.shape[-2:]
    ok = np.isfinite(flat) & (flat > 0)
    val = np.where(ok, flat, np.float32(np.inf))
    low = np.full_like(flat, np.inf)
    bad = np.zeros(flat.shape, dtype=bool)
    for dy in range(-e, e + 1):
        for dx in range(-e, e + 1):
            ys, yd = slice(max(dy, 0), h + min(dy, 0)), slice(max(-dy, 0), h + min(-dy, 0))
            xs, xd = slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0))
            low[:, yd, xd] = np.minimum(low[:, yd, xd], val[:, ys, xs])
            bad[:, yd, xd] |= ~ok[:, ys, xs]
    return np.where(bad, np.float32(0), low).astype(np.float32).reshape(d.shape)


def oracle_volume(O, grid, index_offset=(0, 0, 0), nvox=None, axes=None):
    """An OracleVolume that only classifies: the axis tables of the box (``index_offset``, ``nvox``) of ``grid``'s lattice --
    (index + offset) * voxel_size + origin, the reference's expression (clipfusion.py:617-622) -- or the tables ``axes`` as given."""
    nvox = tuple(int(v) for v in (grid.nvox if nvox is None else nvox))
    vol = O.OracleVolume(grid.origin, grid.voxel_size, torch.tensor(nvox), grid.trunc, 1)
    origin = torch.as_tensor(grid.origin, dtype=torch.float32)
    if axes is None:
        axes = [(torch.arange(nvox[a]) + int(index_offset[a])) * grid.voxel_size + origin[a] for a in range(3)]
    vol.axes = [torch.as_tensor(a).detach().cpu().to(torch.float32).contiguous() for a in axes]
    assert [len(a) for a in vol.axes] == list(nvox)
    return vol


def evidence(vol, depth, poses, K, weight, seen=None, hit=None):
    """``seen`` / ``hit`` int32[N] after the frames ``depth`` [B,H,W] (as the pass gets them: already eroded), ``poses`` [B,4,4],
    ``K`` [B,3,3]: seen += sum_f [(m & 2) and not (m & 1)], hit += sum_f [m & 1], where ``weight > 0``; other entries stay."""
    weight = np.asarray(weight).reshape(-1)
    seen = np.zeros(weight.size, dtype=np.int32) if seen is None else np.array(seen, dtype=np.int32)
    hit = np.zeros(weight.size, dtype=np.int32) if hit is None else np.array(hit, dtype=np.int32)
    depth = torch.as_tensor(np.asarray(depth), dtype=torch.float32)
    h, w = depth.shape[-2:]
    rgb, feat = torch.zeros(h, w, 3), torch.zeros(1, 1, 1)
    touched = weight > 0
    for f in range(depth.shape[0]):
        m, _ = vol.classify(depth[f], rgb, torch.as_tensor(poses[f]), torch.as_tensor(K[f]), feat)
        valid, tsdf_valid = (m & 1) != 0, (m & 2) != 0
        seen += (touched & tsdf_valid & ~valid).astype(np.int32)
        hit += (touched & valid).astype(np.int32)
    return seen, hit


def decide(weight, seen, hit, min_views, max_support):
    """(carved bool[N], counts [touched, carved, kept for support, kept for too few views])."""
    weight, seen, hit = (np.asarray(a).reshape(-1) for a in (weight, seen, hit))
    touched = weight > 0
    enough = touched & (seen >= min_views)
    carved = enough & (hit <= max_support)
    supported = enough & (hit > max_support)
    few = touched & (seen > 0) & (seen < min_views)
    return carved, [int(touched.sum()), int(carved.sum()), int(supported.sum()), int(few.sum())]


def carve(bufs, carved):
    """The volume's buffers (name -> array whose first axis is the voxel; floats as their BIT PATTERNS or as values) with every
    carved voxel zeroed in all of them; the others byte for byte what they were."""
    out = {}
    for name, a in bufs.items():
        a = np.array(a, copy=True)
        a[carved] = 0
        out[name] = a
    return out
