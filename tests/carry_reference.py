"""The NumPy statement of saf_volume_carry (include/saf.h) that the tests of ``move_grid`` hold the device pass to, with slices.

A volume is a dict of arrays shaped by its grid: ``tsdf``, ``tsdf_weight``, ``weight`` [nx,ny,nz], ``rgb`` [nx,ny,nz,3],
``clip_feat`` [nx,ny,nz,D] (any dtype: values are copied, never computed with), optionally ``labels_one_hot`` [nx,ny,nz,C] and
``aux`` [nx,ny,nz].  Destination voxel (x, y, z) corresponds to source voxel (x + off).  Every comparison against it is exact."""
import numpy as np

SMALL = ("tsdf", "tsdf_weight", "weight", "rgb")
ROWS = ("clip_feat", "labels_one_hot")


def overlap(src_nvox, dst_nvox, off):
    """(slices into dst, slices into src) of the overlap, or None when the boxes share no voxel."""
    d, s = [], []
    for n_s, n_d, o in zip(src_nvox, dst_nvox, off):
        lo, hi = max(0, -o), min(n_d, n_s - o)
        if hi <= lo:
            return None
        d.append(slice(lo, hi))
        s.append(slice(lo + o, hi + o))
    return tuple(d), tuple(s)


def carry(src, dst, off):
    """``dst`` (modified in place) after the pass, and (rows carried, tsdf voxels carried).  Small fields over the overlap; rows
    where the source ``weight`` is > 0 -- no other row of ``src`` is read, no other row of ``dst`` written."""
    ov = overlap(src["weight"].shape, dst["weight"].shape, off)
    if ov is None:
        return dst, (0, 0)
    d, s = ov
    for name in SMALL + (("aux",) if "aux" in src else ()):
        dst[name][d] = src[name][s]
    touched = src["weight"][s] > 0
    for name in ROWS:
        if name in src:
            view = dst[name][d]  # (basic slices: a view)
            view[touched] = src[name][s][touched]
    return dst, (int(touched.sum()), int((src["tsdf_weight"][s] > 0).sum()))


def written_masks(src, dst_nvox, off):
    """Boolean [nx,ny,nz] masks over the destination: voxels of the overlap, and those among them whose rows are carried."""
    inside = np.zeros(tuple(dst_nvox), dtype=bool)
    rows = np.zeros(tuple(dst_nvox), dtype=bool)
    ov = overlap(src["weight"].shape, dst_nvox, off)
    if ov is not None:
        d, s = ov
        inside[d] = True
        rows[d] = src["weight"][s] > 0
    return inside, rows
